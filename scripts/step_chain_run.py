#!/usr/bin/env python3
"""Drive the C3 step (bench.py's default workload and plan) with early bootstraps on or off, to be run under a profiler's
kernel trace: bench.py has no switch for `abn_plan_set_early_bootstraps`.

    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -- python scripts/step_chain_run.py --early 0

Prints one JSON line: the mode, the steps and the host-clock milliseconds per step (under a tracer: not a benchmark figure).
scripts/step_chain_table.py turns the trace into the segment table of docs/experiments.md ("Early bootstraps")."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--early", type=int, default=1, choices=[0, 1])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import numpy as np

    import alphabeta_rs_amd as A
    from alphabeta_rs_amd import synthetic

    A.load_library()
    ped, p0 = synthetic.c3_pedigree()
    with A.Context(0) as ctx:
        plan = A.Plan(ctx, ped[:, :3], 1, 10, 10000, options=A.default_options(seed=20260101))
        plan.set_early_bootstraps(args.early)
        plan.set_windows(ped[:, 3][None, :], np.array([p0]))
        for _ in range(args.warmup):
            plan.run()
        plan.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            plan.run()
        plan.sync()
        ms = 1e3 * (time.perf_counter() - t0) / args.steps
        eb = plan.early_bootstraps()
        plan.close()
    print(json.dumps({"early": args.early, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
                      "early_bootstraps": {k: int(v) for k, v in eb.items()}}))


if __name__ == "__main__":
    main()
