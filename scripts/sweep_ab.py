#!/usr/bin/env python3
"""A/B of the stream sweep (abn_plan_set_stream_sweep: a streamed chain's rows read once per Nelder-Mead iteration by
abn_sweep_kernel instead of once per cost evaluation by the stream form of abn_fit_kernel), in one process:

  per shape one plan per mode (0 = per-evaluation kernel, 1 = sweep), the two run alternately, --warmup (1) + --reps (10)
  times; a host clock around run() + sync(), kernel_ms() per phase, counters() and stream_sweep()["passes"] beside them.
  Before anything is timed the two modes' downloads are compared byte for byte.

Shapes:
  c5_sm0, c5_sm1   the C5 pedigree (N = 20 100, T = 125, K = 950: the deep loop), 1 window x --starts (10) x --boot (8192),
                   at stream_mode 0 (materialised bootstrap observations) and 1 (index row + residual gather)
  mid_sm0          a mid-size streamed pedigree (N = --mid-rows (2000) at T = 12: the pair-loop variant), 10 starts x
                   --mid-boot (4096): three power tables per iteration may well lose here

Baseline = mode 0 of the same build.  The rule for a later change of the default, per variant (deep loop / pair loop): on
where the sweep's median is below mode 0's by more than the larger of the two interquartile ranges.  Prints one JSON line
and writes it to --out (default profiles/sweep_ab.json)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))      # _parity.synthetic_pedigree: the tests' random valid pedigree

NOT_MEASURED = [
    "traffic past L2 (FETCH_SIZE / WRITE_SIZE) of either mode: no counter run was made, so the ratio of traffic to "
    "algorithmic bytes that would stand beside the per-evaluation kernel's 2.0x is not known",
    "occupancy actually reached by the sweep kernel's workgroups (LDS allows four per CU on C5) and its stall reasons",
    "more than one window, window groups, several devices",
    "a two-candidate variant (reflection + contraction in the pass, the expansion evaluated on its own)",
    "other depths of the deep loop than 12 row blocks in flight per lane",
]


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    q1, med, q3 = np.percentile(xs, [25, 50, 75])
    return {"median": float(med), "iqr": float(q3 - q1), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def measure(A, ctx, name, ped, p0, S, B, stream_mode, reps, warmup):
    o = A.default_options(stream_mode=stream_mode)
    plans = []
    for mode in (0, 1):
        plan = A.Plan(ctx, ped[:, :3], 1, S, B, options=o)
        plan.set_stream_sweep(mode)
        plan.set_windows(ped[:, 3][None, :], np.array([p0]))
        plans.append(plan)
    outs = []
    for plan in plans:                                 # the comparison run (not timed)
        plan.run()
        outs.append(plan.download())
    for k in ("models", "pred", "resid", "raw", "info_a", "info_b", "best_start"):
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), (name, k)
    res = {"shape": name, "n_rows": int(ped.shape[0]), "tmax": int(ped[:, :3].max()), "starts": S, "boot": B,
           "stream_mode": stream_mode, "downloads_equal": True, "reps": reps, "warmup": warmup}
    host = ([], [])
    kms = ({"fit_starts": [], "fit_boot": []}, {"fit_starts": [], "fit_boot": []})
    for rep in range(warmup + reps):
        for mode, plan in enumerate(plans):
            t0 = time.perf_counter()
            plan.run()
            plan.sync()
            dt = (time.perf_counter() - t0) * 1e3
            k = plan.kernel_ms()
            if rep >= warmup:
                host[mode].append(dt)
                for ph in kms[mode]:
                    kms[mode][ph].append(float(k[ph]))
    for mode, plan in enumerate(plans):
        cnt, sw, kinds = plan.counters(), plan.stream_sweep(), plan.last_kernels()
        res[f"mode{mode}"] = {"run_ms": stats(host[mode]), "fit_starts_ms": stats(kms[mode]["fit_starts"]),
                              "fit_boot_ms": stats(kms[mode]["fit_boot"]), "kernels": {k: list(v) for k, v in kinds.items()},
                              "counters": {k: int(v) for k, v in cnt.items()}, "stream_sweep": sw,
                              "fits_per_s_boot": B / (stats(kms[mode]["fit_boot"])["median"] * 1e-3)}
        plan.close()
    assert res["mode1"]["kernels"]["boot"][0] == "stream_sweep" and res["mode0"]["kernels"]["boot"][0] == "stream", res
    for key in ("run_ms", "fit_starts_ms", "fit_boot_ms"):
        a, b = res["mode0"][key], res["mode1"][key]
        res[f"{key}_sweep_over_mode0"] = b["median"] / a["median"]
        res[f"{key}_sweep_faster_beyond_the_larger_iqr"] = bool(b["median"] < a["median"] - max(a["iqr"], b["iqr"]))
    res["passes_over_evals"] = res["mode1"]["stream_sweep"]["passes"] / res["mode1"]["counters"]["evals"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--starts", type=int, default=10)
    ap.add_argument("--boot", type=int, default=8192)
    ap.add_argument("--mid-rows", type=int, default=2000)
    ap.add_argument("--mid-boot", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10, help="10 for a measurement; fewer for a functional run, marked as such")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="c5_sm0,c5_sm1,mid_sm0")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "sweep_ab.json")
    args = ap.parse_args()
    if args.reps < 1 or args.warmup < 1:
        ap.error("--reps >= 1, --warmup >= 1")
    import alphabeta_rs_amd as A
    from alphabeta_rs_amd import synthetic
    from _parity import synthetic_pedigree

    A.load_library(build_if_missing=True)
    if A.device_count() <= 0:
        sys.exit("no HIP device: nothing to time")
    ctx = A.Context(0)
    info = {"tool": "scripts/sweep_ab.py", "fewer_than_10_reps_a_functional_run_only": args.reps < 10,
            "baseline": "mode 0 of the same build", "shapes": [], "not_measured": NOT_MEASURED,
            "rule": "default on for a variant (deep loop / pair loop) where the sweep's median is below mode 0's by more "
                    "than the larger interquartile range"}
    c5, p5 = synthetic.c5_pedigree()
    mid = synthetic_pedigree(np.random.default_rng(2), args.mid_rows, 12)
    for name in args.shapes.split(","):
        if name in ("c5_sm0", "c5_sm1"):
            r = measure(A, ctx, name, c5, p5, args.starts, args.boot, int(name[-1]), args.reps, args.warmup)
        elif name == "mid_sm0":
            r = measure(A, ctx, name, mid, 0.7, args.starts, args.mid_boot, 0, args.reps, args.warmup)
        else:
            sys.exit(f"unknown shape {name}")
        info["shapes"].append(r)
        print(json.dumps({"shape": name, "run_ms": [r["mode0"]["run_ms"], r["mode1"]["run_ms"]],
                          "fit_boot_ms": [r["mode0"]["fit_boot_ms"], r["mode1"]["fit_boot_ms"]]}), file=sys.stderr, flush=True)
    ctx.close()
    print(json.dumps(info), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(info) + "\n")


if __name__ == "__main__":
    main()
