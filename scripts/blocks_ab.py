#!/usr/bin/env python3
"""What the block bootstrap's kernels cost (abn_block_*, alphabeta_rs_amd/csrc/abn_blocks.hpp), next to the serial host form
on the same inputs.

Per shape (T blocks, pairs, R replicates; one group; 2^14-sized table values, so three digits) the counts are drawn on the
device (abn_block_counts: wall time, the copy of G x (R + 1) x T bytes to the host included), then sent up once and the
tables resampled through the device-pointer entry abn_block_resample_dev --warmup + --reps times: the HIP-event times of
digits, product, finish and levels (what abn_tiles_block_ms reports for a handle) and the entry's wall time, medians of the
timed calls.  abn_block_resample_host runs on the same tables and the first --host-rows rows of the same counts on one core
of the GPU host; its time per row times the number of rows is the serial figure the kernels are compared against (an
extrapolation, and marked as one: the whole serial run of the largest shape is hours).  The rows the host form computed
are compared with the device's, integer for integer, before anything is reported.

Shapes: (1 200, 45, 1 000), (12 000, 1 225, 1 000), (120 000, 1 225, 10 000); a shape whose buffers do not fit the device's
free memory is reported as skipped.  --scale shrinks T and R (rehearsal).  Without a device the script stops after checking
the host form against itself (no CPU fallback exists).  Prints one JSON line per shape and writes them to --out (default
profiles/blocks_ab.json).
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = [(1_200, 45, 1_000), (12_000, 1_225, 1_000), (120_000, 1_225, 10_000)]
SAMPLES = {45: 10, 1_225: 50}


def tables(T, P, n, seed):
    rng = np.random.default_rng(seed)
    both = rng.integers(1 << 10, 1 << 14, size=(T, P), dtype=np.uint64)
    diff = (both // rng.integers(2, 40, size=(T, P), dtype=np.uint64)).astype(np.uint64)
    lsk = rng.random((n, T)) * 1000.0
    kept = rng.integers(500, 2000, size=(n, T)).astype(np.int64)
    return both, diff, lsk, kept


def run_shape(T, P, R, args, A, torch, ctx):
    n = SAMPLES.get(P, 2)
    rows = R + 1
    need = rows * T + 2 * 8 * T * P + 2 * 5 * (T + 64) * (P + 16) + 3 * 8 * rows * P + 2 * 8 * rows * n + 16 * n * T
    free = torch.cuda.mem_get_info()[0]
    line = {"blocks": T, "pairs": P, "replicates": R, "samples": n, "device_bytes": int(need)}
    if need > 0.8 * free:
        return {**line, "skipped": f"needs {need} bytes, {free} free"}
    both, diff, lsk, kept = tables(T, P, n, 20261 + T)
    gb, ge = np.array([0], dtype=np.int64), np.array([T], dtype=np.int64)
    t0 = time.perf_counter()
    counts = ctx.block_counts(args.seed, [0], gb, ge, R, T)
    line["counts_wall_ms"] = (time.perf_counter() - t0) * 1e3
    assert counts[0, :, :].sum(axis=1, dtype=np.int64).tolist() == [T] * rows
    dev = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda() for a in (counts, both, diff, lsk, kept)]
    out = [torch.zeros((rows, P), dtype=torch.int64, device="cuda"), torch.zeros((rows, P), dtype=torch.int64, device="cuda"),
           torch.zeros((rows, P), dtype=torch.float64, device="cuda"), torch.zeros((rows, n), dtype=torch.float64, device="cuda"),
           torch.zeros((rows, n), dtype=torch.int64, device="cuda")]
    ms, wall = [], []
    for k in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = ctx.block_resample_dev(gb, ge, rows, dev[0].data_ptr(), T, P, n, *(d.data_ptr() for d in dev[1:]),
                                   *(o.data_ptr() for o in out))
        w = (time.perf_counter() - t0) * 1e3
        if k >= args.warmup:
            ms.append(m), wall.append(w)
    med = np.median(np.array(ms), axis=0)
    line.update({"digits_ms": med[1], "product_ms": med[2], "finish_ms": med[3], "levels_ms": med[4],
                 "kernels_ms": float(med[1:].sum()), "wall_ms": statistics.median(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall),
                 "multiply_adds": 2 * rows * T * P, "reps": args.reps})
    h = min(args.host_rows, rows)
    part = np.ascontiguousarray(np.concatenate([counts[:, :h - 1], counts[:, R:]], axis=1))       # some replicates and the identity row
    t0 = time.perf_counter()
    host = A.block_resample_host(gb, ge, part, both, diff, lsk, kept)
    host_ms = (time.perf_counter() - t0) * 1e3
    pick = list(range(h - 1)) + [R]
    for key, o in zip(("both", "diff", "dvalue", "level", "kept"), out):
        got = o[pick].cpu().numpy()
        assert got.tobytes() == host[key][0].view(got.dtype).tobytes(), key
    line.update({"host_rows": h, "host_ms_measured": host_ms, "host_ms_all_rows_extrapolated": host_ms / h * rows})
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-rows", type=int, default=8)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=20260101)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "blocks_ab.json"))
    args = ap.parse_args()
    import torch  # before the product library: one HIP runtime in the process (as bench.py)

    import alphabeta_rs_amd as A

    small = tables(300, 3, 2, 1)
    c = A.block_counts_host(args.seed, [0], [0], [300], 4, 300)
    a, b = A.block_resample_host([0], [300], c, *small), A.block_resample_host([0], [300], c.copy(), *small)
    assert all(a[k].tobytes() == b[k].tobytes() for k in a) and int(a["both"][0, 4].sum()) == int(small[0].sum())
    if A.device_count() <= 0:
        print("no HIP device: the host form was checked, nothing was timed")
        return
    ctx = A.Context(0)
    lines = []
    for T, P, R in SHAPES:
        T, R = max(int(T * args.scale), 64), max(int(R * args.scale), 1)
        lines.append(run_shape(T, P, R, args, A, torch, ctx))
        print(json.dumps(lines[-1]), flush=True)
    ctx.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
