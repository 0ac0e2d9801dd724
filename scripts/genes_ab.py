#!/usr/bin/env python3
"""A/B of the gene choice of `metaprofile --methylome`, in one process, alternating, from the parsed FullSite vectors of
every methylome to the finished windows::Handle (counts, sums and the packed matrix resident):

  (a) windows::choose_genes per methylome on 16 threads (the serial loop with its last-gene cache, six push_backs per
      site), the samples' arrays concatenated, abn_windows_create — the stage as it is with --genes host;
  (b) the site fields concatenated, abn_genes_create + abn_windows_create_sites: one upload, the gene of every site chosen
      by the three kernels of csrc/abn_genes.hpp, the placement fed from the device arrays — what --genes device runs.

Both are timed with a host clock around the whole span (both end in device synchronisations); the HIP-event times of the
three kernels (abn_genes_choose on the same sites) are reported beside them.  The shape: --samples (8) methylomes of
--sites (2 000 000) CG rows each on five chromosomes, both strands, positions ascending, over a synthetic annotation of
--genes (30 000) genes of both strands; the samples share their coordinates (two distinct texts, used in turn: what differs
between real samples, status and level, does not enter the gene choice).  Before anything is timed the two handles are
compared: counts, sums bit for bit, layout and packed bytes.

"(b) is not slower" = its median is not above (a)'s by more than the larger of the two interquartile ranges; that decides
the default of --genes.  Prints one JSON line and writes it to --out (default profiles/genes_ab.json).
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
CHROMOSOMES = 5


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    q1, med, q3 = np.percentile(xs, [25, 50, 75])
    return {"median": float(med), "iqr": float(q3 - q1), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def annotation(n_genes, span, seed):
    """genes of 200 to 6000 bp, both strands, spread over the chromosomes; neighbours overlap here and there"""
    rng = np.random.default_rng(seed)
    chrom = rng.integers(1, CHROMOSOMES + 1, size=n_genes)
    start = rng.integers(3000, span, size=n_genes)
    end = start + rng.integers(200, 6000, size=n_genes)
    strand = np.where(rng.integers(0, 2, size=n_genes) == 0, "+", "-")
    return "".join(f"{c}\t{a}\t{b}\tG{i}\tx\t{s}\n" for i, (c, a, b, s) in enumerate(zip(chrom, start, end, strand))).encode()


def methylome(n_sites, span, seed):
    """CG rows, the chromosomes one after the other, positions ascending inside each, a random strand per row"""
    rng = np.random.default_rng(seed)
    per = n_sites // CHROMOSOMES
    chrom = np.repeat(np.arange(1, CHROMOSOMES + 1), per)
    pos = np.concatenate([np.sort(rng.integers(1, span + 8000, size=per)) for _ in range(CHROMOSOMES)])
    n = len(pos)
    strand = np.where(rng.integers(0, 2, size=n) == 0, "+", "-")
    pm = np.char.mod("%.4f", np.where(rng.random(n) < 0.8, 0.99 + 0.0099 * rng.random(n), rng.random(n)))
    lvl = np.char.mod("%.4f", rng.random(n))
    st = np.array(list("UIM"))[rng.integers(0, 3, size=n)]
    cols = chrom.astype(str), pos.astype(str), strand, ["CG"] * n, ["3"] * n, ["8"] * n, pm, st, lvl, ["CGA"] * n
    return (HEADER + "\n".join("\t".join(r) for r in zip(*cols)) + "\n").encode()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--genes", type=int, default=30_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "genes_ab.json")
    args = ap.parse_args()
    if args.reps < 10 or args.warmup < 1:
        ap.error("--reps >= 10, --warmup >= 1")
    import alphabeta_rs_amd as A
    from alphabeta_rs_amd import build as B

    A.load_library(build_if_missing=True)
    B.build_host()
    if A.device_count() <= 0:
        sys.exit("no HIP device: both sides end in abn_windows_*, nothing to time")
    L = C.CDLL(str(B.PEDIGREE_LIB))
    ll, dp = C.c_longlong, C.POINTER(C.c_double)
    L.abh_windows_handles_ab.argtypes = [C.c_char_p, ll, C.POINTER(C.c_char_p), C.POINTER(ll), C.c_int, C.c_uint, C.c_int,
                                         C.c_double, C.c_uint, C.c_uint, C.c_int, C.c_int, C.c_int, dp, dp]
    span = 24_000_000          # per chromosome: 120 Mb in all, a gene every 4 kb, a CG row every 60 bp
    t0 = time.perf_counter()
    ann = annotation(args.genes, span, 7)
    distinct = [methylome(args.sites, span, 100 + k) for k in range(min(2, args.samples))]
    texts = [distinct[s % len(distinct)] for s in range(args.samples)]
    info = {"samples": args.samples, "sites_per_sample": int(distinct[0].count(b"\n") - 1), "genes": args.genes,
            "chromosomes": CHROMOSOMES, "cutoff": 2048, "step": 5, "size": 5, "absolute": False, "threads": args.threads,
            "reps": args.reps, "warmup": args.warmup, "generate_s": round(time.perf_counter() - t0, 1)}
    print(json.dumps(info), file=sys.stderr, flush=True)
    ptrs = (C.c_char_p * len(texts))(*texts)
    lens = (ll * len(texts))(*map(len, texts))
    ms2, ms3 = (C.c_double * 2)(), (C.c_double * 3)()

    def call(n, which):
        rc = L.abh_windows_handles_ab(ann, len(ann), ptrs, lens, n, 2048, 0, 0.99, 5, 5, 0, args.threads, which, ms2, ms3)
        assert rc == 1, f"abh_windows_handles_ab: {rc} (0: the two handles differ)"
        return ms2[0], ms2[1], list(ms3)

    t0 = time.perf_counter()
    call(len(texts), 3)                                   # parses and keeps the sites; compares the two handles
    info["equal"], info["parse_and_compare_s"] = True, round(time.perf_counter() - t0, 1)
    print(json.dumps(info), file=sys.stderr, flush=True)
    host, dev, kernels = [], [], []
    for rep in range(args.warmup + args.reps):
        h, _, _ = call(0, 1)
        _, d, _ = call(0, 2)
        _, _, k = call(0, 4)
        if rep >= args.warmup:
            host.append(h)
            dev.append(d)
            kernels.append(k)
    info["host_ms"], info["device_ms"] = stats(host), stats(dev)
    for i, name in enumerate(("find", "carry", "write")):
        info[f"kernel_ms_{name}"] = stats([k[i] for k in kernels])
    margin = max(info["host_ms"]["iqr"], info["device_ms"]["iqr"])
    info["device_not_slower_within_the_larger_iqr"] = bool(info["device_ms"]["median"] <= info["host_ms"]["median"] + margin)
    print(json.dumps(info), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(info) + "\n")


if __name__ == "__main__":
    main()
