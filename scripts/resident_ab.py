#!/usr/bin/env python3
"""A/B of where the parsed sites of `metaprofile --methylome` wait for the gene choice, in one process, alternating, from
the methylome texts in host memory to the finished windows::Handle (counts, sums and the packed matrix resident):

  (a) windows::parse_sites_many on the device — per methylome the upload of its text, the five kernels, the download of
      the records, the merge with the deferred lines into FullSite vectors — then site_arrays and
      abn_windows_create_sites: the records come down, are copied twice on the host and go up again.  What
      --parse device --genes device --sites host runs;
  (b) windows::parse_sites_resident per methylome — the same upload and kernels, only the deferred triples and the
      flagged lines come back, the accepted deferred lines go up (abn_sites_insert) — then abn_windows_create_parsed: the
      two merge kernels of csrc/abn_sites_merge.hpp write the arrays of the gene choice in place.  What --sites device runs.

Both are timed with a host clock around the whole span (both end in device synchronisations); the HIP-event times of (b)'s
two merge kernels (abn_windows_merge_ms) are reported beside them.  Shapes: `lines` = --samples-lines (15) all-context
methylomes of --lines (1 000 000) lines, about one in seven CG, over the bundled annotation (the shape of
scripts/parse_ab.py); `lines_deferring` = the same with the posterior of every 14th CG line (1 % of all lines) spelled with 23
digits, which the device defers and the host accepts; `cg` = --samples-cg (8) methylomes of --sites (2 000 000) CG rows on five
chromosomes over a synthetic annotation of 30 000 genes (the shape of scripts/genes_ab.py).  Before anything is timed the
two handles of a shape are compared: counts, sums bit for bit, layout and packed bytes.

"(b) is faster" = its median is below (a)'s by more than the larger of the two interquartile ranges.  Prints one JSON
line and writes it to --out (default profiles/resident_ab.json).
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path


ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

import genes_ab  # noqa: E402  (its annotation and CG-row methylome)
import parse_ab  # noqa: E402  (its all-context methylome)

LONG = "0.99990000000000000000000"


def deferring(text, every):
    """the posterior token of every `every`-th CG line replaced by a spelling the device defers (a line of another context
    is no site whatever its tokens are, and is not deferred)"""
    lines = text.split(b"\n")
    seen = 0
    for i in range(1, len(lines) - 1):
        if b"\tCG\t" in lines[i]:
            seen += 1
            if seen % every == 0:
                f = lines[i].split(b"\t")
                f[6] = LONG.encode()
                lines[i] = b"\t".join(f)
    return b"\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples-lines", type=int, default=15)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--samples-cg", type=int, default=8)
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--genes", type=int, default=30_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "resident_ab.json")
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
    L.abh_windows_resident_ab.argtypes = [C.c_char_p, ll, C.POINTER(C.c_char_p), C.POINTER(ll), C.c_int, C.c_uint, C.c_int,
                                          C.c_double, C.c_uint, C.c_uint, C.c_int, C.c_int, dp, dp]
    stats = genes_ab.stats
    result = {"reps": args.reps, "warmup": args.warmup, "cutoff": 2048, "step": 5, "size": 5, "absolute": False, "shapes": {}}

    def run(name, annotation, texts):
        ptrs = (C.c_char_p * len(texts))(*texts)
        lens = (ll * len(texts))(*map(len, texts))
        ms2, k2 = (C.c_double * 2)(), (C.c_double * 2)()

        def call(n, which):
            rc = L.abh_windows_resident_ab(annotation, len(annotation), ptrs, lens, n, 2048, 0, 0.99, 5, 5, 0, which, ms2, k2)
            assert rc == 1, f"abh_windows_resident_ab: {rc} (0: the two handles differ)"
            return ms2[0], ms2[1], (k2[0], k2[1])

        info = {"samples": len(texts), "text_bytes": int(sum(map(len, texts))), "lines_per_sample": int(texts[0].count(b"\n")),
                "deferring_lines_sample0": int(texts[0].count(LONG.encode()))}
        t0 = time.perf_counter()
        call(len(texts), 3)                               # hands the texts over; compares the two handles
        info["equal"], info["compare_s"] = True, round(time.perf_counter() - t0, 1)
        host, dev, kernels = [], [], []
        for rep in range(args.warmup + args.reps):
            h, _, _ = call(0, 1)
            _, d, k = call(0, 2)
            if rep >= args.warmup:
                host.append(h)
                dev.append(d)
                kernels.append(k)
        info["host_ms"], info["resident_ms"] = stats(host), stats(dev)
        info["kernel_ms_fields"], info["kernel_ms_insert"] = stats([k[0] for k in kernels]), stats([k[1] for k in kernels])
        margin = max(info["host_ms"]["iqr"], info["resident_ms"]["iqr"])
        info["resident_faster_beyond_the_larger_iqr"] = bool(info["resident_ms"]["median"] < info["host_ms"]["median"] - margin)
        info["resident_not_slower_within_the_larger_iqr"] = bool(info["resident_ms"]["median"] <= info["host_ms"]["median"] + margin)
        result["shapes"][name] = info
        print(json.dumps({name: info}), file=sys.stderr, flush=True)

    t0 = time.perf_counter()
    annotation = (ROOT / "tests" / "golden" / "annotation.txt").read_bytes()
    genes = [(int(f[0]), int(f[1]), int(f[2])) for f in (l.split(b"\t") for l in annotation.splitlines()) if f[0] == b"1"]
    texts = [parse_ab.methylome(args.lines, 100 + s, genes) for s in range(args.samples_lines)]
    result["generate_lines_s"] = round(time.perf_counter() - t0, 1)
    run("lines", annotation, texts)
    t0 = time.perf_counter()
    texts = [deferring(t, 14) for t in texts]
    result["generate_deferring_s"] = round(time.perf_counter() - t0, 1)
    run("lines_deferring", annotation, texts)
    del texts
    t0 = time.perf_counter()
    span = 24_000_000
    synthetic = genes_ab.annotation(args.genes, span, 7)
    distinct = [genes_ab.methylome(args.sites, span, 100 + k) for k in range(min(2, args.samples_cg))]
    result["generate_cg_s"] = round(time.perf_counter() - t0, 1)
    run("cg", synthetic, [distinct[s % len(distinct)] for s in range(args.samples_cg)])
    print(json.dumps(result), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
