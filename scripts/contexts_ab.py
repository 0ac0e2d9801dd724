#!/usr/bin/env python3
"""What one device parse of every methylome under all three contexts buys (abn_sites_params.contexts, abn_sites_split).

Three questions on all-context methylomes as the golden files are (the rows of tests/_parse_model.plain_text), each
methylome parsed into a resident handle, interleaved repetitions in one process on one device:

  1. the CG-only resident parse: kernel_ms of another build of the library (--parent-lib: the commit before contexts)
     against contexts = CG of this one — expected equal;
  2. one parse under CG|CHG|CHH plus the split against three times the other build's single parse: the least three
     separate runs would cost;
  3. the split's two kernels alone: bytes moved per second (count: the 4-byte meta word of every record; scatter: 32 bytes
     read and 32 written per record and child).

Both builds are driven through the same raw ctypes calls.  Writes one JSON document (--out) and prints it.
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
HEADER = ("seqnames\tstart\tstrand\tcontext\tcounts.methylated\tcounts.total\tposteriorMax\tstatus\trc.meth.lvl\t"
          "context.trinucleotide\n")


class SitesParams(C.Structure):
    _fields_ = [("slab_bytes", C.c_int64), ("skip_lines", C.c_int32), ("contexts", C.c_int32)]


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    q1, med, q3 = np.percentile(xs, [25, 50, 75])
    return {"median": float(med), "iqr": float(q3 - q1), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def methylome(n_lines, seed, cg_every=7):
    """plain_text's rows, the columns drawn at once: one line in cg_every is CG, the rest CHH or CHG, four-decimal values"""
    rng = np.random.default_rng(seed)
    ctx = np.where(rng.integers(cg_every, size=n_lines) == 0, 0, 1 + rng.integers(2, size=n_lines))
    cols = zip((1 + np.arange(n_lines) // 1000000).tolist(), range(1, n_lines + 1), rng.integers(2, size=n_lines).tolist(),
               ctx.tolist(), rng.integers(30, size=n_lines).tolist(), rng.integers(30, 60, size=n_lines).tolist(),
               rng.random(n_lines).tolist(), rng.integers(3, size=n_lines).tolist(), rng.random(n_lines).tolist())
    names = ("CG", "CHH", "CHG")
    body = "".join(f"{c}\t{p}\t{'+-'[s]}\t{names[x]}\t{m}\t{t}\t{pm:.4f}\t{'UIM'[st]}\t{ml:.4f}\tCGA\n"
                   for c, p, s, x, m, t, pm, st, ml in cols)
    return (HEADER + body).encode()


class Lib:
    """one build of the library behind the calls both builds have; split only where it exists"""

    def __init__(self, path, device):
        self.L = L = C.CDLL(str(path))
        vp = C.c_void_p
        L.abn_init.argtypes = [C.c_int, vp, C.POINTER(vp)]
        L.abn_shutdown.argtypes = [vp]
        L.abn_sites_parse_dev.argtypes = [vp, C.c_char_p, C.c_int64, C.POINTER(SitesParams), C.POINTER(vp)]
        L.abn_sites_info.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        L.abn_sites_destroy.argtypes = [vp]
        self.has_split = hasattr(L, "abn_sites_split")
        if self.has_split:
            L.abn_sites_split.argtypes = [vp, C.POINTER(vp)]
            L.abn_sites_split_ms.argtypes = [vp, C.POINTER(C.c_double)]
        self.ctx = vp()
        assert L.abn_init(device, None, C.byref(self.ctx)) == 0

    def close(self):
        self.L.abn_shutdown(self.ctx)

    def run(self, texts, contexts, split):
        """every text parsed into a resident handle (and split) -> {kernel_ms, split_ms[2], wall_ms, records, deferred}"""
        out = {"kernel_ms": 0.0, "count_ms": 0.0, "scatter_ms": 0.0, "records": 0, "deferred": 0, "child_records": 0}
        t0 = time.perf_counter()
        for text in texts:
            h, p = C.c_void_p(), SitesParams(0, 0, contexts)
            assert self.L.abn_sites_parse_dev(self.ctx, text, len(text), C.byref(p), C.byref(h)) == 0
            n, nd, ms = C.c_int64(), C.c_int64(), C.c_double()
            self.L.abn_sites_info(h, C.byref(n), C.byref(nd), None, C.byref(ms))
            out["kernel_ms"] += ms.value
            out["records"] += n.value
            out["deferred"] += nd.value
            if split:
                kids, ms2 = (C.c_void_p * 3)(), (C.c_double * 2)()
                assert self.L.abn_sites_split(h, kids) == 0
                self.L.abn_sites_split_ms(h, ms2)
                out["count_ms"] += ms2[0]
                out["scatter_ms"] += ms2[1]
                for k in kids:
                    kn = C.c_int64()
                    self.L.abn_sites_info(k, C.byref(kn), None, None, None)
                    out["child_records"] += kn.value
                    self.L.abn_sites_destroy(k)
            self.L.abn_sites_destroy(h)
        out["wall_ms"] = (time.perf_counter() - t0) * 1e3
        return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-lib", default="", help="libabneutral_hip.so of the commit before contexts; none: questions 1 and 2 have no other side")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "contexts_ab.json"))
    args = ap.parse_args()
    from alphabeta_rs_amd import build as B

    B.build_hip()
    texts = [methylome(args.lines, seed=1000 + s) for s in range(args.samples)]
    sides = {"branch_cg": (Lib(B.LIB, args.device), 0, False), "branch_all_split": None}
    sides["branch_all_split"] = (sides["branch_cg"][0], 7, True)
    if args.parent_lib:
        sides = {"parent_cg": (Lib(args.parent_lib, args.device), 0, False), **sides}
        assert not sides["parent_cg"][0].has_split, "--parent-lib already has abn_sites_split"
    for lib, contexts, split in sides.values():                              # warm-up: the pools, the code objects
        lib.run(texts[:1], contexts, split)
    runs = {k: [] for k in sides}
    for _ in range(max(args.reps, 5)):                                       # interleaved
        for k, (lib, contexts, split) in sides.items():
            runs[k].append(lib.run(texts, contexts, split))
    doc = {"samples": args.samples, "lines_per_sample": args.lines, "text_bytes": int(sum(len(t) for t in texts)),
           "reps": len(runs["branch_cg"]), "sides": {}}
    for k, rs in runs.items():
        doc["sides"][k] = {"records": rs[0]["records"], "deferred": rs[0]["deferred"],
                           "kernel_ms": stats([r["kernel_ms"] for r in rs]), "wall_ms": stats([r["wall_ms"] for r in rs])}
    a = runs["branch_all_split"]
    n, moved = a[0]["records"], a[0]["child_records"]
    assert moved == n, "every record of an all-context methylome belongs to one child"
    doc["split"] = {"count_ms": stats([r["count_ms"] for r in a]), "scatter_ms": stats([r["scatter_ms"] for r in a]),
                    "count_bytes": 4 * n, "scatter_bytes": 64 * moved,
                    "count_gb_per_s": stats([4 * n / r["count_ms"] / 1e6 for r in a]),
                    "scatter_gb_per_s": stats([64 * moved / r["scatter_ms"] / 1e6 for r in a])}
    one = [r["kernel_ms"] + r["count_ms"] + r["scatter_ms"] for r in a]
    doc["one_parse_plus_split_kernel_ms"] = stats(one)
    if args.parent_lib:
        p = runs["parent_cg"]
        doc["three_parent_parses_kernel_ms"] = stats([3 * r["kernel_ms"] for r in p])
        doc["three_parent_parses_wall_ms"] = stats([3 * r["wall_ms"] for r in p])
        doc["cg_parse_branch_over_parent"] = doc["sides"]["branch_cg"]["kernel_ms"]["median"] / doc["sides"]["parent_cg"]["kernel_ms"]["median"]
        doc["one_parse_over_three"] = doc["one_parse_plus_split_kernel_ms"]["median"] / doc["three_parent_parses_kernel_ms"]["median"]
        doc["one_parse_over_three_wall"] = doc["sides"]["branch_all_split"]["wall_ms"]["median"] / doc["three_parent_parses_wall_ms"]["median"]
    for lib in {id(v[0]): v[0] for v in sides.values()}.values():
        lib.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
