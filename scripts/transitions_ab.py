#!/usr/bin/env python3
"""What the 3 x 3 state transition scan costs next to the divergence scan on the same resident packed matrix, in one
process, alternating.

Per shape the seeded random codes of scripts/pairwise_packed_ab.py are packed on the device; the kernels' HIP-event time
(kernel_ms) of abn_pairwise_transitions_packed_dev and of abn_pairwise_divergence_packed_dev is taken --warmup + --reps
times, the two alternating so that both see the same box; the median of the timed calls is reported, with its spread, and
the ratio transitions / divergence.  By instruction count the transitions scan does nine matrix products where the
divergence scan does three, on the same bytes: a ratio of about 3 is the expectation to compare against.

Shapes: the four `pw` shapes of bench.py (15 x 4 M, 15 x 32 M, 50 x 32 M, 50 x 2 M sites) and one tiles shape — 8 samples,
2 M sites, 1000 tiles of 2000 columns each — through the two windows entries (abn_pairwise_transitions_windows_packed_dev,
abn_pairwise_divergence_windows_packed_dev).  --scale shrinks every length (rehearsal).

Before anything is timed the table is folded to `both` and `diff` and compared with the divergence scan's, integer for
integer.  Without a device the script stops after checking the host packing (no CPU fallback exists).  Prints one JSON line
per shape and writes them to --out (default profiles/transitions_ab.json).
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

import pairwise_packed_ab as PP  # noqa: E402  (its codes, its packing, its statistics)

SHAPES = [(15, 4_000_000), (15, 32_000_000), (50, 32_000_000), (50, 2_000_000)]   # bench.py: PAIRWISE_SHAPES
TILES_SHAPE = (8, 2_000_000, 2000)                                                # samples, sites, columns per tile


def run_shape(n, L, tile, args, A, torch, ctx):
    stride = A.packed_row_stride(L)
    npairs = n * (n - 1) // 2
    codes = PP.device_codes(torch, n, L, 20261 + n)
    packed = PP.device_pack(torch, codes, stride)
    del codes
    if tile:
        begin = np.arange(0, L - tile + 1, tile, dtype=np.int64)
        end = begin + tile
    W = len(begin) if tile else 1
    table = torch.zeros((W, npairs, 9), dtype=torch.int64, device="cuda")
    diff, both = (torch.zeros((W, npairs), dtype=torch.int64, device="cuda") for _ in range(2))
    dval = torch.zeros((W, npairs), dtype=torch.float64, device="cuda")

    def trans():
        if tile:
            return ctx.pairwise_transitions_windows_packed_dev(packed.data_ptr(), n, L, stride, begin, end, table.data_ptr())
        return ctx.pairwise_transitions_packed_dev(packed.data_ptr(), n, L, stride, table.data_ptr())

    def div():
        if tile:
            return ctx.pairwise_divergence_windows_packed_dev(packed.data_ptr(), n, L, stride, begin, end, diff.data_ptr(),
                                                              both.data_ptr(), dval.data_ptr())
        return ctx.pairwise_divergence_packed_dev(packed.data_ptr(), n, L, stride, diff.data_ptr(), both.data_ptr(),
                                                  dval.data_ptr())

    torch.cuda.synchronize()   # the library's stream is not torch's: the inputs are complete before a scan reads them
    trans(), div()
    torch.cuda.synchronize()
    weight = torch.tensor([0, 1, 2, 1, 0, 1, 2, 1, 0], dtype=torch.int64, device="cuda")
    assert torch.equal(table.sum(dim=2), both) and torch.equal((table * weight).sum(dim=2), diff) and int(both.max()) > 0

    t = {"transitions": [], "divergence": []}
    for rep in range(args.warmup + args.reps):
        row = {"transitions": trans(), "divergence": div()}
        if rep >= args.warmup:
            for k, v in row.items():
                t[k].append(v)
    res = {k: PP.stats(v) for k, v in t.items()}
    return {"samples": n, "sites": L, "tiles": W if tile else None, "columns_per_tile": tile or None,
            "row_stride_bytes": stride, "code_bytes": n * stride, "kernel_ms": res,
            "ratio_transitions_over_divergence": res["transitions"]["median"] / res["divergence"]["median"],
            "expected_ratio_by_matrix_instructions": 3.0}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every length (0.01: a rehearsal)")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "transitions_ab.json")
    args = ap.parse_args()
    if args.reps < 1 or args.warmup < 0 or not 0 < args.scale <= 1:
        ap.error("--reps >= 1, --warmup >= 0, 0 < --scale <= 1")
    import torch  # before the product library: one HIP runtime in the process (as bench.py)

    import alphabeta_rs_amd as A

    A.load_library(build_if_missing=True)
    lines = []
    if A.device_count() <= 0:
        print("no HIP device: host packing and oracle only", file=sys.stderr)
        lines.append(PP.rehearse(A))
        print(json.dumps(lines[-1]), flush=True)
    else:
        with A.Context(0) as ctx:
            for n, L, tile in [(n, L, 0) for n, L in SHAPES] + [TILES_SHAPE]:
                info = run_shape(n, int(L * args.scale), tile, args, A, torch, ctx)
                info.update({"reps": args.reps, "warmup": args.warmup, "scale": args.scale})
                lines.append(info)
                print(json.dumps(info), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
