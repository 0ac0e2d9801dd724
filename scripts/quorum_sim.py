#!/usr/bin/env python3
"""Development aid (CPU only, on the oracle): how often the best of S starts is among the first q to finish, and how many
iterations of phase A a launch of phase B at that quorum saves — the hit table behind route_early_bootstraps' quorum
(docs/experiments.md, "Early bootstraps").  Windows: synthetic.c4_windows (the C3 topology with window-specific rates),
10 starts each, the canonical tree.  A start that runs into argmin's fixed point counts as finishing at once: the
device's fixed-point skip ends it on the spot.

    python scripts/quorum_sim.py [windows = 120] [starts = 10]"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import oracle as O
from alphabeta_rs_amd import synthetic

SEED, CANON, MAX_ITERS = 20260101, 0x10040, 10000


def window_lengths(w, starts):
    """(iterations of each start on the device's clock, index of the best start) of window w"""
    gens, D, p0, _ = synthetic.c4_windows(1, window_offset=w)
    ped = np.concatenate([gens, D[0][:, None]], axis=1)
    s0 = np.stack([O.start_simplex(SEED, w, s, float(D[0].max())) for s in range(starts)])
    fits = O.fit_batch(ped, p0[0], p0[0], 1.0, s0, MAX_ITERS, lanes=CANON)
    best = O.select_best(ped, p0[0], fits["best"])[0]
    stuck = (fits["status"] == 1) & (fits["iters"] == MAX_ITERS)
    return np.where(stuck, 0, fits["iters"]), int(best)


def main():
    windows = int(sys.argv[1]) if len(sys.argv) > 1 else 120
    starts = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    O.build()
    cases = [window_lengths(w, starts) for w in range(windows)]
    longest = np.array([ln.max() for ln, _ in cases])
    print(f"{windows} windows x {starts} starts; mean longest chain {longest.mean():.0f} iterations")
    print("| q | best is among the first q | mean iterations saved on a hit | mean saved per window (a miss saves 0) |")
    print("|---|---|---|---|")
    for q in range(starts - 1, starts // 2, -1):
        hits, saved = 0, []
        for ln, best in cases:
            order = np.argsort(ln, kind="stable")
            if best in order[:q]:
                hits += 1
                saved.append(ln.max() - ln[order[q - 1]])
        print(f"| {q} | {hits} / {windows} | {np.mean(saved):.0f} | {np.sum(saved) / windows:.0f} |")


if __name__ == "__main__":
    main()
