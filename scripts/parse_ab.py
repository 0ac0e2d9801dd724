#!/usr/bin/env python3
"""A/B of the methylome parse stage of `metaprofile --methylome`, in one process, alternating:

  (a) windows::choose_genes_many: every line of every methylome through the host's parser (split, a string per field,
      strtod), one methylome per thread on 16 threads, with the gene choice — the stage as it is without --parse device;
  (b) windows::choose_genes_many_device: abn_sites_parse per methylome (upload, the five kernels, download), the merge
      with the deferred lines and the gene choice — what --parse device runs.

Both are timed with a host clock around the whole call (b ends in device synchronisations); the kernels' HIP-event time
(abn_sites_info) of one methylome is reported beside them.  The shape: --samples (15) methylomes of --lines (1 000 000)
lines each, all-context, about one line in seven CG, four-decimal values as in the bundled methylomes, seeded.  Before
anything is timed the two results are compared array for array, bit for bit.

"(b) is faster" = its median is below (a)'s by more than the larger of the two interquartile ranges; that decides the
default of --parse.  Without a device the script stops after building the texts and checking the host parser against the
shared line parser on one of them.  Prints one JSON line and writes it to --out (default profiles/parse_ab.json).
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


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    q1, med, q3 = np.percentile(xs, [25, 50, 75])
    return {"median": float(med), "iqr": float(q3 - q1), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def methylome(n_lines, seed, genes):
    """all-context rows over the annotation's first genes and their flanks, positions ascending per chromosome"""
    rng = np.random.default_rng(seed)
    lo = min(g[1] for g in genes) - 2000
    pos = lo + np.arange(n_lines, dtype=np.int64) * 3 + rng.integers(0, 3, size=n_lines)
    ctx = np.where(rng.integers(0, 7, size=n_lines) == 0, "CG", np.where(rng.integers(0, 2, size=n_lines) == 0, "CHH", "CHG"))
    strand = np.where(rng.integers(0, 2, size=n_lines) == 0, "+", "-")
    total = rng.integers(1, 60, size=n_lines)
    meth = (total * rng.random(n_lines)).astype(np.int64)
    pm = np.char.mod("%.4f", np.where(rng.random(n_lines) < 0.8, 0.99 + 0.0099 * rng.random(n_lines), rng.random(n_lines)))
    lvl = np.char.mod("%.4f", rng.random(n_lines))
    st = np.array(list("UIM"))[rng.integers(0, 3, size=n_lines)]
    tri = np.array(["CGA", "CCT", "CAG", "CTG"])[rng.integers(0, 4, size=n_lines)]
    cols = ["1"] * n_lines, pos.astype(str), strand, ctx, meth.astype(str), total.astype(str), pm, st, lvl, tri
    return (HEADER + "\n".join("\t".join(r) for r in zip(*cols)) + "\n").encode()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "parse_ab.json")
    args = ap.parse_args()
    if args.reps < 10 or args.warmup < 1:
        ap.error("--reps >= 10, --warmup >= 1")
    import alphabeta_rs_amd as A
    from alphabeta_rs_amd import build as B

    A.load_library(build_if_missing=True)
    B.build_host()
    L = C.CDLL(str(B.PEDIGREE_LIB))
    ll = C.c_longlong
    L.abh_choose_genes_many_ab.argtypes = [C.c_char_p, ll, C.POINTER(C.c_char_p), C.POINTER(ll), C.c_int, C.c_uint,
                                           C.c_double, C.c_int, C.c_int, C.POINTER(C.c_double)]
    annotation = (ROOT / "tests" / "golden" / "annotation.txt").read_bytes()
    genes = [(int(f[0]), int(f[1]), int(f[2])) for f in (l.split(b"\t") for l in annotation.splitlines()) if f[0] == b"1"]
    t0 = time.perf_counter()
    texts = [methylome(args.lines, 100 + s, genes) for s in range(args.samples)]
    info = {"samples": args.samples, "lines_per_sample": args.lines, "text_bytes": int(sum(map(len, texts))),
            "cg_lines": int(sum(t.count(b"\tCG\t") for t in texts)), "threads": args.threads, "reps": args.reps,
            "warmup": args.warmup, "generate_s": None}
    info["generate_s"] = round(time.perf_counter() - t0, 1)
    has_device = A.device_count() > 0
    ptrs = (C.c_char_p * len(texts))(*texts)
    lens = (ll * len(texts))(*map(len, texts))
    ms2 = (C.c_double * 2)()

    def call(n, which):
        rc = L.abh_choose_genes_many_ab(annotation, len(annotation), ptrs, lens, n, 2048, 0.99, args.threads, which, ms2)
        assert rc == 1, f"abh_choose_genes_many_ab: {rc} (0: the two sides differ)"
        return ms2[0], ms2[1]

    if not has_device:
        call(len(texts), 1)
        info["device"] = None
        print("no HIP device: texts and the host side only", file=sys.stderr)
        print(json.dumps(info))
        return
    call(len(texts), 3)                                   # hands the texts over; compares the two sides bit for bit
    info["bit_equal"] = True
    with A.Context(0) as ctx:
        sites, deferred = ctx.parse_sites(texts[0])
        kernel = []
        for _ in range(args.warmup + args.reps):
            kernel.append(ctx.parse_sites(texts[0])[0]["kernel_ms"])
        info["sites_sample0"], info["deferred_sample0"] = int(len(sites["line"])), int(len(deferred["line"]))
        info["kernel_ms_one_methylome"] = stats(kernel[args.warmup:])
    host, dev = [], []
    for rep in range(args.warmup + args.reps):
        h, _ = call(0, 1)
        _, d = call(0, 2)
        if rep >= args.warmup:
            host.append(h)
            dev.append(d)
    info["host_ms"], info["device_ms"] = stats(host), stats(dev)
    margin = max(info["host_ms"]["iqr"], info["device_ms"]["iqr"])
    info["device_faster_beyond_the_larger_iqr"] = bool(info["device_ms"]["median"] < info["host_ms"]["median"] - margin)
    print(json.dumps(info), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(info) + "\n")


if __name__ == "__main__":
    main()
