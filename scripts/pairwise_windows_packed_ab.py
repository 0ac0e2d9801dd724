#!/usr/bin/env python3
"""A/B of the windows scan on 2-bit packed codes against the windows scan on byte codes, in one process, alternating:

  (a) abn_pairwise_divergence_windows      on the byte code matrix;
  (b) abn_pairwise_divergence_windows_packed on abn_pack_codes of the same matrix, the same windows.

Two timings each: the kernels' HIP-event time of the device-resident entries (codes and results in HBM), and a host clock
around the synchronising host-buffer entries (uploads and downloads included; the packing itself is done once, before).
The baseline is (a) of the same run.  "Not slower" = (b)'s median is within the larger of the two interquartile ranges of
(a)'s median.

Shapes: the two seeded ones of scripts/pairwise_windows_ab.py — "meta" = 15 samples, 200 windows of 20 000 - 200 000
sites laid side by side; "long" = 50 samples, 60 windows of 1 - 2 M sites over rows of 16 M sites.  --scale shrinks every
length (rehearsal).  Kernel time: --kernel-reps (>= 30) repetitions; host entries: --reps-meta (>= 30) and --reps-long
(>= 5) — the long shape uploads 0.8 GB per byte call.

Before anything is timed the two entries are compared bit for bit on the timed inputs (and with the oracle on the first
windows).  Without a device the script stops after building the shapes and checking the oracle on them (no CPU fallback
exists).  Prints one JSON line per shape and writes them to --out (default profiles/pairwise_windows_packed_ab.json).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from pairwise_windows_ab import make_shape, oracle_check  # noqa: E402  (the shapes are that script's, seeds included)


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    q1, med, q3 = np.percentile(xs, [25, 50, 75])
    return {"median": float(med), "iqr": float(q3 - q1), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def compare(a, b):
    """(b) against the baseline (a): the ratio of the medians, and whether (b) is within the larger IQR of (a)"""
    return {"ratio_b_over_a": b["median"] / a["median"],
            "b_not_slower_than_a": bool(b["median"] <= a["median"] + max(a["iqr"], b["iqr"]))}


def run_shape(name, args, A, torch, ctx):
    n, codes, begin, end = make_shape(name, args.scale)
    W, npairs, sites = len(begin), n * (n - 1) // 2, codes.shape[1]
    info = {"shape": name, "samples": n, "windows": W, "sites_per_row": sites, "byte_matrix_bytes": int(codes.nbytes),
            "window_sites": int((end - begin).sum()), "min_sites": int((end - begin).min()),
            "max_sites": int((end - begin).max())}
    if ctx is None:
        oracle_check(codes, begin, end)
        info["device"] = None
        return info
    packed = A.pack_codes(codes)
    stride = packed.shape[1]
    info["packed_matrix_bytes"] = int(packed.nbytes)

    def a_host():
        return ctx.pairwise_divergence_windows(codes, begin, end)

    def b_host():
        return ctx.pairwise_divergence_windows_packed(packed, sites, begin, end)

    # the two entries agree bit for bit on the timed inputs (and with the oracle on the first windows)
    ra, rb = a_host(), b_host()
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2], equal_nan=True)
    assert rb[1].max() > 0
    oracle_check(codes, begin, end, rb)

    dev = torch.device("cuda:0")
    d_codes, d_packed = torch.from_numpy(codes).to(dev), torch.from_numpy(packed).to(dev)
    assert d_packed.data_ptr() % 16 == 0
    d_a = [torch.zeros((W, npairs), dtype=torch.int64, device=dev), torch.zeros((W, npairs), dtype=torch.int64, device=dev),
           torch.zeros((W, npairs), dtype=torch.float64, device=dev)]
    d_b = [torch.zeros_like(o) for o in d_a]

    def a_dev():
        return ctx.pairwise_divergence_windows_dev(d_codes.data_ptr(), n, sites, begin, end, *(o.data_ptr() for o in d_a))

    def b_dev():
        return ctx.pairwise_divergence_windows_packed_dev(d_packed.data_ptr(), n, sites, stride, begin, end,
                                                          *(o.data_ptr() for o in d_b))

    a_dev(), b_dev()
    torch.cuda.synchronize()
    assert torch.equal(d_a[0], d_b[0]) and torch.equal(d_a[1], d_b[1])
    assert np.array_equal(d_a[2].cpu().numpy(), d_b[2].cpu().numpy(), equal_nan=True)
    assert np.array_equal(d_b[0].cpu().numpy().view(np.uint64), rb[0])

    t = {"a_kernel_ms": [], "b_kernel_ms": [], "a_host_ms": [], "b_host_ms": []}
    for rep in range(args.warmup + args.kernel_reps):
        row = {"a_kernel_ms": a_dev(), "b_kernel_ms": b_dev()}
        if rep >= args.warmup:
            for k, v in row.items():
                t[k].append(v)
    host_reps = args.reps_meta if name == "meta" else args.reps_long
    for rep in range(args.warmup + host_reps):
        row = {}
        for key, fn in (("a_host_ms", a_host), ("b_host_ms", b_host)):
            t0 = time.perf_counter()
            fn()
            row[key] = (time.perf_counter() - t0) * 1e3
        if rep >= args.warmup:
            for k, v in row.items():
                t[k].append(v)
    res = {k: stats(v) for k, v in t.items()}
    info.update(res)
    info["kernel"] = compare(res["a_kernel_ms"], res["b_kernel_ms"])
    info["host"] = compare(res["a_host_ms"], res["b_host_ms"])
    return info


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", choices=("meta", "long", "both"), default="both")
    ap.add_argument("--kernel-reps", type=int, default=30)
    ap.add_argument("--reps-meta", type=int, default=30)
    ap.add_argument("--reps-long", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every length (0.01: a rehearsal)")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "pairwise_windows_packed_ab.json")
    args = ap.parse_args()
    if args.kernel_reps < 30 or args.reps_meta < 30 or args.reps_long < 5 or args.warmup < 1 or not 0 < args.scale <= 1:
        ap.error("--kernel-reps >= 30, --reps-meta >= 30, --reps-long >= 5, --warmup >= 1, 0 < --scale <= 1")
    import torch  # before the product library: one HIP runtime in the process (as bench.py)

    import alphabeta_rs_amd as A

    A.load_library(build_if_missing=True)
    ctx = A.Context(0) if A.device_count() > 0 else None
    if ctx is None:
        print("no HIP device: shapes and oracle only", file=sys.stderr)
    lines = []
    for name in (("meta", "long") if args.shape == "both" else (args.shape,)):
        info = run_shape(name, args, A, torch, ctx)
        info.update({"kernel_reps": args.kernel_reps, "host_reps": args.reps_meta if name == "meta" else args.reps_long,
                     "warmup": args.warmup, "scale": args.scale})
        lines.append(info)
        print(json.dumps(info), flush=True)
    if ctx is not None:
        ctx.close()
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
