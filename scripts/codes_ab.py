#!/usr/bin/env python3
"""A/B of where the parsed sites of `alphabeta -n nodelist -e edgelist --parse device` wait for the pedigree build, in one
process, alternating, from the methylome texts in host memory to the finished pedigree and p0uu (Pedigree::build without
its file reads):

  (a) --sites host: per methylome abn_sites_parse — the upload of its text, the kernels, the download of the six record
      arrays (32 B per site), the merge with the deferred lines — the copy into Site vectors (24 B per site), the
      rc_meth_lvl fold and write_codes_packed on the host, the upload of the packed matrix, the scan;
  (b) --sites device: per methylome abn_sites_parse_dev — the same upload and kernels, only the deferred triples and the
      flagged lines come back, the accepted deferred lines go up (abn_sites_insert) — then abn_codes_create_parsed (the
      reduced merge, the pack and the fold kernels of csrc/abn_codes.hpp) and abn_codes_pairwise on the resident matrix.

Both are timed with a host clock around the whole span (both end in device synchronisations); the HIP-event times of (b)'s
four kernels (abn_codes_kernel_ms: merge of the records, merge of the inserted lines, pack, fold) are reported beside
them.  Shapes, those of scripts/resident_ab.py: `lines` = --samples-lines (15) all-context methylomes of --lines
(1 000 000) lines, about one in seven CG, cut to one number of CG rows (the surplus CG rows of a sample, from its end, are
given another context: Pedigree::build scans samples of one length); `lines_deferring` = the same with the posterior of
every 14th CG line (1 % of all lines) spelled with 23 digits, which the device defers and the host accepts; `cg` =
--samples-cg (8) methylomes of --sites (2 000 000) CG rows.  The pedigree is a chain: sample s is generation s.  Before
anything is timed the two results of a shape are compared: the pedigree's rows and p0uu, bit for bit.

"(b) is faster" = its median is below (a)'s by more than the larger of the two interquartile ranges.  Prints one JSON
line and writes it to --out (default profiles/codes_ab.json).
"""
import argparse
import ctypes as C
import json
import sys
import tempfile
import time
from pathlib import Path


ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

import genes_ab  # noqa: E402  (its CG-row methylome)
import parse_ab  # noqa: E402  (its all-context methylome)
from resident_ab import LONG, deferring  # noqa: E402


def one_length(texts):
    """every text with the CG rows of the one that has the fewest: the last surplus CG rows of the others become CHG rows"""
    counts = [t.count(b"\tCG\t") for t in texts]
    return [b"\tCHG\t".join(t.rsplit(b"\tCG\t", c - min(counts))) if c > min(counts) else t for t, c in zip(texts, counts)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples-lines", type=int, default=15)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--samples-cg", type=int, default=8)
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "codes_ab.json")
    args = ap.parse_args()
    if args.reps < 10 or args.warmup < 1:
        ap.error("--reps >= 10, --warmup >= 1")
    import alphabeta_rs_amd as A
    from alphabeta_rs_amd import build as B

    A.load_library(build_if_missing=True)
    B.build_host()
    if A.device_count() <= 0:
        sys.exit("no HIP device: both sides parse on the device, nothing to time")
    L = C.CDLL(str(B.PEDIGREE_LIB))
    ll, dp = C.c_longlong, C.POINTER(C.c_double)
    L.abh_pedigree_build_ab.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(ll), C.c_int, C.c_double,
                                        C.c_int, dp, dp, C.c_char_p, C.c_int]
    stats = genes_ab.stats
    result = {"reps": args.reps, "warmup": args.warmup, "posterior_max_filter": 0.99, "shapes": {}}
    tmp = Path(tempfile.mkdtemp(prefix="codes_ab_"))

    def run(name, texts):
        n = len(texts)
        nodes, edges = tmp / f"{name}_nodelist.txt", tmp / f"{name}_edgelist.txt"
        nodes.write_text("filename,node,gen,meth\n" + "".join(f"memory_{s},s{s},{s},Y\n" for s in range(n)))
        edges.write_text("from\tto\tgendiff\n" + "".join(f"s{s}\ts{s + 1}\t1\n" for s in range(n - 1)))
        ptrs = (C.c_char_p * n)(*texts)
        lens = (ll * n)(*map(len, texts))
        ms2, k4, err = (C.c_double * 2)(), (C.c_double * 4)(), C.create_string_buffer(512)

        def call(k, which):
            rc = L.abh_pedigree_build_ab(str(nodes).encode(), str(edges).encode(), ptrs, lens, k, 0.99, which, ms2, k4, err, 512)
            assert rc == 1, f"abh_pedigree_build_ab: {rc} (0: the two results differ) {err.value!r}"
            return ms2[0], ms2[1], tuple(k4)

        info = {"samples": n, "text_bytes": int(sum(map(len, texts))), "lines_per_sample": int(texts[0].count(b"\n")),
                "sites_per_sample": int(texts[0].count(b"\tCG\t")), "deferring_lines_sample0": int(texts[0].count(LONG.encode()))}
        t0 = time.perf_counter()
        call(n, 3)                                        # hands the texts over; compares the two results
        info["equal"], info["compare_s"] = True, round(time.perf_counter() - t0, 1)
        host, dev, kernels = [], [], []
        for rep in range(args.warmup + args.reps):
            h, _, _ = call(0, 1)
            _, d, k = call(0, 2)
            if rep >= args.warmup:
                host.append(h)
                dev.append(d)
                kernels.append(k)
        info["host_ms"], info["device_ms"] = stats(host), stats(dev)
        for i, key in enumerate(("merge_records", "merge_inserted", "pack", "fold")):
            info[f"kernel_ms_{key}"] = stats([k[i] for k in kernels])
        margin = max(info["host_ms"]["iqr"], info["device_ms"]["iqr"])
        info["device_faster_beyond_the_larger_iqr"] = bool(info["device_ms"]["median"] < info["host_ms"]["median"] - margin)
        info["device_not_slower_within_the_larger_iqr"] = bool(info["device_ms"]["median"] <= info["host_ms"]["median"] + margin)
        result["shapes"][name] = info
        print(json.dumps({name: info}), file=sys.stderr, flush=True)

    t0 = time.perf_counter()
    annotation = (ROOT / "tests" / "golden" / "annotation.txt").read_bytes()
    genes = [(int(f[0]), int(f[1]), int(f[2])) for f in (l.split(b"\t") for l in annotation.splitlines()) if f[0] == b"1"]
    texts = one_length([parse_ab.methylome(args.lines, 100 + s, genes) for s in range(args.samples_lines)])
    result["generate_lines_s"] = round(time.perf_counter() - t0, 1)
    run("lines", texts)
    t0 = time.perf_counter()
    texts = [deferring(t, 14) for t in texts]
    result["generate_deferring_s"] = round(time.perf_counter() - t0, 1)
    run("lines_deferring", texts)
    del texts
    t0 = time.perf_counter()
    distinct = [genes_ab.methylome(args.sites, 24_000_000, 100 + k) for k in range(min(2, args.samples_cg))]
    result["generate_cg_s"] = round(time.perf_counter() - t0, 1)
    run("cg", [distinct[s % len(distinct)] for s in range(args.samples_cg)])
    print(json.dumps(result), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
