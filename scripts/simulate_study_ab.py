#!/usr/bin/env python3
"""What a replicate study costs on the device (abn_sim_study), kernel by kernel, next to what it replaces.

Per shape (nodes V, sites per replicate L, replicates R), every node emitted, E = 0.02 and F = 0.1:
  - ms4 of simulate.study: the HIP-event ms of the simulation of R L sites, the observation in place, the packed windows
    scan over the R ranges and the census; 2 warm-up calls, then --repeats, median and quartiles;
  - the HIP-event ms of simulate.codes_dev on the same shape (V nodes, R L sites): the simulation alone, for the ratio
    observation per emitted row : simulation per node (here every node is a row, so the ratio of the two times);
  - the wall ms of one study call, and the wall ms of R calls of simulate.pedigree(L) — the host loop the study stands in
    for (no observation step: the loop has none) — with the sum of their HIP-event ms.
Nothing is asserted.  Writes one JSON document (--out) and prints its rows.
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
SHAPES = [(8, 100_000, 16), (8, 100_000, 128), (8, 1_000_000, 32), (100, 100_000, 32), (100, 1_000_000, 8)]


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    q1, med, q3 = np.percentile(xs, [25, 50, 75])
    return {"median": float(med), "q1": float(q1), "q3": float(q3), "n": int(xs.size)}


def tree(V):
    """V nodes, node v the child of (v - 1) // 2, two generations per level"""
    parent = [-1] + [(v - 1) // 2 for v in range(1, V)]
    generation = [0] * V
    for v in range(1, V):
        generation[v] = generation[parent[v]] + 2
    return parent, generation, [1] * V


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "simulate_study_ab.json"))
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    import alphabeta_rs_amd as abn
    from alphabeta_rs_amd import simulate as S

    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    ctx = abn.Context(0)
    rates = (2e-3, 5e-3, 0.7, 0.3)
    miscall, dropout = S.noise(0.02, 0.1)
    rows = []
    for V, L, R in SHAPES:
        parent, generation, emit = tree(V)
        study = lambda: S.study(ctx, 20260101, parent, generation, emit, *rates, L, R, miscall=miscall, dropout=dropout, with_ms=True)
        for _ in range(2):
            study()
        ms, wall = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            ms.append(study()[4])
            wall.append(1e3 * (time.perf_counter() - t0))
        ms = np.array(ms)
        thr = S.thresholds(parent, generation, *rates)
        stride = abn.packed_row_stride(R * L)
        buf = C.c_void_p()
        assert hip.hipMalloc(C.byref(buf), V * stride) == 0
        codes = lambda: S.codes_dev(ctx, 20260101, parent, thr, emit, R * L, buf.value, stride)
        for _ in range(2):
            codes()
        codes_ms = [codes() for _ in range(a.repeats)]
        hip.hipFree(buf)

        def loop():
            t0, kernel = time.perf_counter(), 0.0
            for r in range(R):
                kernel += float(S.pedigree(ctx, 20260101 + r, parent, generation, emit, *rates, L, with_ms=True)[2].sum())
            return 1e3 * (time.perf_counter() - t0), kernel

        loop()
        loops = [loop() for _ in range(3)]
        row = {"nodes": V, "sites": L, "replicates": R, "sim_ms": stats(ms[:, 0]), "obs_ms": stats(ms[:, 1]), "scan_ms": stats(ms[:, 2]),
               "census_ms": stats(ms[:, 3]), "codes_dev_ms": stats(codes_ms), "study_wall_ms": stats(wall),
               "loop_wall_ms": stats([x[0] for x in loops]), "loop_kernel_ms": stats([x[1] for x in loops])}
        row["obs_per_row_over_sim_per_node"] = row["obs_ms"]["median"] / row["sim_ms"]["median"]
        rows.append(row)
        print(f"V {V:>3d} L {L:>8d} R {R:>4d}  sim {row['sim_ms']['median']:.3f}  obs {row['obs_ms']['median']:.3f}  scan "
              f"{row['scan_ms']['median']:.3f}  census {row['census_ms']['median']:.3f}  codes_dev {row['codes_dev_ms']['median']:.3f}  "
              f"obs/sim {row['obs_per_row_over_sim_per_node']:.3f}  study wall {row['study_wall_ms']['median']:.2f}  loop wall "
              f"{row['loop_wall_ms']['median']:.2f} (kernels {row['loop_kernel_ms']['median']:.2f})", flush=True)
    ctx.close()
    Path(a.out).parent.mkdir(exist_ok=True)
    Path(a.out).write_text(json.dumps({"rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
