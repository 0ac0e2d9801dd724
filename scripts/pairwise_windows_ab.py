#!/usr/bin/env python3
"""A/B of the batched window scan against the loop it replaces, in one process, alternating:

  (a) a loop of abn_pairwise_divergence over the windows, each on its own contiguous copy of its columns — what
      Pedigree::build did once per metaprofile window;
  (b) one abn_pairwise_divergence_windows call over the code matrix.

Two timings each: a host clock around the synchronising host-buffer entries (uploads and downloads included), and the
kernels' HIP-event time of the device-resident entries (codes and results in HBM).  The baseline is (a) of the same run.

Shapes (seeded): "meta" = 15 samples, 200 windows, lengths log-uniform in 20 000 - 200 000 sites, laid side by side in one
matrix as Pedigree::build_many does; "long" = 50 samples, 60 windows of 1 - 2 M sites sliding over rows of 16 M sites (the
chunked path against the single-window kernel at a comparable length).  --scale shrinks every length (rehearsal).

Without a device the script stops after building the shapes and checking the oracle on them (no CPU fallback exists).
Prints one JSON line per shape; --out writes them to a file as well.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def make_shape(name, scale, seed=20261):
    rng = np.random.default_rng(seed)
    if name == "meta":
        n, W = 15, 200
        lens = np.exp(rng.uniform(np.log(20_000 * scale), np.log(200_000 * scale), size=W)).astype(np.int64)
        begin = np.concatenate([[0], np.cumsum((lens + 127) // 128 * 128)[:-1]]).astype(np.int64)
        stride = int(begin[-1] + (lens[-1] + 127) // 128 * 128)
    else:
        n, W = 50, 60
        lens = rng.integers(int(1_000_000 * scale), int(2_000_000 * scale) + 1, size=W).astype(np.int64)
        stride = int(16_000_000 * scale) + 3
        begin = rng.integers(0, stride - lens.max(), size=W).astype(np.int64)
    codes = rng.integers(0, 3, size=(n, stride), dtype=np.uint8)
    codes |= (rng.random(size=(n, stride), dtype=np.float32) < 0.08).astype(np.uint8) << 7
    return n, codes, begin, begin + lens


def oracle_check(codes, begin, end, got=None, windows=(0, 1)):
    import oracle as O

    O.build()
    for w in windows:
        sl = codes[:, begin[w]:end[w]][:, :50_000]
        wd, wb, wv = O.pairwise_divergence(sl & 3, np.where(sl & 0x80, 0.5, 1.0), 0.99)
        assert wb.max() > 0 and np.all(wd <= 2 * wb)
        if got is not None and end[w] - begin[w] <= 50_000:
            assert np.array_equal(got[0][w], wd) and np.array_equal(got[1][w], wb)
            assert np.array_equal(got[2][w], wv, equal_nan=True)


def stats(xs):
    xs = np.sort(np.asarray(xs, dtype=np.float64))
    med = float(np.median(xs))
    q1, q3 = np.percentile(xs, [25, 75])
    return {"median": med, "min": float(xs[0]), "max": float(xs[-1]), "iqr_over_median": float((q3 - q1) / med),
            "range_over_median": float((xs[-1] - xs[0]) / med), "n": int(xs.size)}


def run_shape(name, args, A, torch, ctx):
    n, codes, begin, end = make_shape(name, args.scale)
    W, npairs, stride = len(begin), n * (n - 1) // 2, codes.shape[1]
    window_bytes = int(n * (end - begin).sum())
    info = {"shape": name, "samples": n, "windows": W, "row_stride": stride, "matrix_bytes": int(codes.nbytes),
            "window_code_bytes": window_bytes, "min_sites": int((end - begin).min()), "max_sites": int((end - begin).max())}
    if ctx is None:
        oracle_check(codes, begin, end)
        info["device"] = None
        return info
    copies = [np.ascontiguousarray(codes[:, b:e]) for b, e in zip(begin, end)]      # (a)'s inputs, made once
    dev = torch.device("cuda:0")
    d_codes = torch.from_numpy(codes).to(dev)
    d_copies = [torch.from_numpy(c).to(dev) for c in copies]
    d_out = [torch.zeros((W, npairs), dtype=torch.int64, device=dev), torch.zeros((W, npairs), dtype=torch.int64, device=dev),
             torch.zeros((W, npairs), dtype=torch.float64, device=dev)]
    d_out_a = [torch.zeros_like(o) for o in d_out]

    def a_host():
        return [ctx.pairwise_divergence(c) for c in copies]

    def b_host():
        return ctx.pairwise_divergence_windows(codes, begin, end)

    def a_dev():
        ms = 0.0
        for w, c in enumerate(d_copies):
            ms += ctx.pairwise_divergence_dev(c.data_ptr(), n, c.shape[1], d_out_a[0][w].data_ptr(),
                                              d_out_a[1][w].data_ptr(), d_out_a[2][w].data_ptr())
        return ms

    def b_dev():
        return ctx.pairwise_divergence_windows_dev(d_codes.data_ptr(), n, stride, begin, end, d_out[0].data_ptr(),
                                                   d_out[1].data_ptr(), d_out[2].data_ptr())

    # the two forms agree bit for bit (and with the oracle on the first windows) before anything is timed
    ra, rb = a_host(), b_host()
    for w in range(W):
        assert np.array_equal(ra[w][0], rb[0][w]) and np.array_equal(ra[w][1], rb[1][w])
        assert np.array_equal(ra[w][2], rb[2][w], equal_nan=True)
    oracle_check(codes, begin, end, rb)
    a_dev(), b_dev()
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(d_out[k], d_out_a[k]) or k == 2
    assert np.array_equal(d_out[2].cpu().numpy(), d_out_a[2].cpu().numpy(), equal_nan=True)
    assert np.array_equal(d_out[0].cpu().numpy().view(np.uint64), rb[0])

    t = {"a_host_ms": [], "b_host_ms": [], "a_kernel_ms": [], "b_kernel_ms": [], "a_dev_wall_ms": [], "b_dev_wall_ms": []}
    for rep in range(args.warmup + args.reps):
        row = {}
        for key, fn in (("a_host_ms", a_host), ("b_host_ms", b_host)):
            t0 = time.perf_counter()
            fn()
            row[key] = (time.perf_counter() - t0) * 1e3
        for key, wall, fn in (("a_kernel_ms", "a_dev_wall_ms", a_dev), ("b_kernel_ms", "b_dev_wall_ms", b_dev)):
            t0 = time.perf_counter()
            row[key] = fn()
            row[wall] = (time.perf_counter() - t0) * 1e3
        if rep >= args.warmup:
            for k, v in row.items():
                t[k].append(v)
    res = {k: stats(v) for k, v in t.items()}
    info.update(res)
    info["ratio_b_over_a"] = {k: res["b_" + k]["median"] / res["a_" + k]["median"] for k in ("host_ms", "kernel_ms", "dev_wall_ms")}
    info["code_GBps_over_kernel_time"] = {s: window_bytes / (res[s + "_kernel_ms"]["median"] * 1e-3) / 1e9 for s in "ab"}
    # (b) is not slower than (a) beyond (a)'s own spread (max - min over its median)
    info["b_not_slower_than_a"] = {k: bool(res["b_" + k]["median"] <= res["a_" + k]["median"] * (1.0 + res["a_" + k]["range_over_median"]))
                                  for k in ("host_ms", "kernel_ms")}
    return info


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shape", choices=("meta", "long", "both"), default="both")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every length (0.01: a rehearsal)")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if args.reps < 1 or args.warmup < 0 or not 0 < args.scale <= 1:
        ap.error("--reps >= 1, --warmup >= 0, 0 < --scale <= 1")
    import torch  # before the product library: one HIP runtime in the process (as bench.py)

    import alphabeta_rs_amd as A

    A.load_library(build_if_missing=True)
    ctx = A.Context(0) if A.device_count() > 0 else None
    if ctx is None:
        print("no HIP device: shapes and oracle only", file=sys.stderr)
    lines = []
    for name in (("meta", "long") if args.shape == "both" else (args.shape,)):
        info = run_shape(name, args, A, torch, ctx)
        info.update({"reps": args.reps, "warmup": args.warmup, "scale": args.scale})
        lines.append(info)
        print(json.dumps(info), flush=True)
    if ctx is not None:
        ctx.close()
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
