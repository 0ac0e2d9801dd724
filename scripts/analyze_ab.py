#!/usr/bin/env python3
"""A/B of the analysis of a plan's bootstrap tables: download + host loop against the device analysis, in one process,
alternating.

Per shape a Plan (the bundled six-row pedigree, --starts starts, B bootstraps, W windows) is run once; then, --warmup +
--reps times and alternating so that both see the same box,
  (a) "host":   Plan.download(want_info=False) — raw[W x B x 7] crosses PCIe — and analyze() of every window's table on
                the host (abn_analyze), what a caller did before Plan.analyze existed;
  (b) "device": Plan.analyze() — abn_plan_analyze: one launch over the table where it lies, W x 32 doubles come back.
Both are timed with the host clock around calls that end in a stream synchronise.  The kernel's own HIP-event time
(abn_analyze_batch_dev on the plan's table) is reported next to them.  Before anything is timed the two results are
compared bit for bit (two NaN count as equal).

Shapes: metaprofile (W = 300, B = 100 and B = 1000), BASELINE C3 (W = 1, B = 10 000), a C4 shard (W = 25, B = 1000).
The condition for the metaprofile driver: at the two metaprofile shapes the median of (b) is not above the median of (a)
by more than (a)'s own interquartile range.  W = 1 is reported, not a condition (one workgroup per column: the serial
Welford chain, one true f64 division per bootstrap, is all there is).

Without a device the script stops after checking the host analysis against the oracle on a small table (no CPU fallback
exists).  Prints one JSON line per shape; --out writes them too.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = [("metaprofile", 300, 100), ("metaprofile", 300, 1000), ("c3", 1, 10_000), ("c4_shard", 25, 1000)]
CONDITION = {("metaprofile", 300, 100), ("metaprofile", 300, 1000)}


def stats(xs):
    xs = np.sort(np.asarray(xs, dtype=np.float64))
    q1, q3 = np.percentile(xs, [25, 75])
    return {"median": float(np.median(xs)), "min": float(xs[0]), "max": float(xs[-1]), "q1": float(q1), "q3": float(q3),
            "iqr": float(q3 - q1), "n": int(xs.size)}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def rehearse(A):
    import oracle as O

    O.build()
    rng = np.random.default_rng(1)
    raw = rng.uniform(0.01, 0.99, (41, 7))
    assert same_bits(A.analyze(raw), O.analyze(raw))
    return {"device": None, "rehearsal": "host analysis equals the oracle's on a 41 x 7 table"}


def run_shape(name, W, B, args, A, O, ctx, torch):
    ped = O.load_pedigree(ROOT / "tests" / "golden" / "pedigree_generated.txt")
    p0 = 0.6554051647850447
    rng = np.random.default_rng(100 + W)
    D = np.tile(ped[:, 3], (W, 1))
    D[1:] = np.abs(D[1:] * rng.uniform(0.7, 1.3, (W - 1, 1)))
    plan = A.Plan(ctx, ped[:, :3], W, args.starts, B, options=A.default_options(seed=7))
    try:
        plan.set_windows(D, np.full(W, p0))
        plan.run()
        plan.sync()

        def host():
            t0 = time.perf_counter()
            raw = plan.download(want_info=False, allow_failed_windows=True)["raw"]
            t1 = time.perf_counter()
            out = np.stack([A.analyze(raw[w]).reshape(32) for w in range(W)])
            return out, (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

        def device():
            t0 = time.perf_counter()
            out, fb = plan.analyze()
            return out, fb, (time.perf_counter() - t0) * 1e3

        want, _, _ = host()
        got, fb, _ = device()
        assert np.all(fb == -1) and same_bits(got, want), "the device analysis differs from the host's"
        dout = torch.zeros(W * 32, dtype=torch.float64, device="cuda")   # the kernel alone, on the table where it lies
        torch.cuda.synchronize()

        def kernel():
            return ctx.analyze_batch_dev(plan.raw_device_ptr(), W, B, dout.data_ptr())

        kernel()
        assert same_bits(dout.cpu().numpy(), want)
        t = {"host": [], "host_download": [], "host_analyze": [], "device": [], "kernel": []}
        for rep in range(args.warmup + args.reps):
            _, dl, an = host()
            _, _, dev = device()
            km = kernel()
            if rep >= args.warmup:
                t["kernel"].append(km)
                t["host"].append(dl + an)
                t["host_download"].append(dl)
                t["host_analyze"].append(an)
                t["device"].append(dev)
        res = {k: stats(v) for k, v in t.items()}
        info = {"shape": name, "windows": W, "bootstraps": B, "starts": args.starts, "table_bytes": W * B * 7 * 8,
                "result_bytes": W * 32 * 8, "ms": res,
                "ratio_device_over_host": res["device"]["median"] / res["host"]["median"],
                "device_within_host_iqr": bool(res["device"]["median"] <= res["host"]["median"] + res["host"]["iqr"]),
                "is_condition": (name, W, B) in CONDITION, "bit_identical": True}
        return info
    finally:
        plan.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--starts", type=int, default=4, help="starts per window of the run that fills the table")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if args.reps < 1 or args.warmup < 0 or args.starts < 1:
        ap.error("--reps >= 1, --warmup >= 0, --starts >= 1")
    import torch  # before the product library: one HIP runtime in the process (as bench.py)

    import alphabeta_rs_amd as A
    import oracle as O

    A.load_library(build_if_missing=True)
    lines = []
    if A.device_count() <= 0:
        print("no HIP device: host analysis against the oracle only", file=sys.stderr)
        lines.append(rehearse(A))
        print(json.dumps(lines[-1]), flush=True)
    else:
        with A.Context(0) as ctx:
            for name, W, B in SHAPES:
                info = run_shape(name, W, B, args, A, O, ctx, torch)
                info.update({"reps": args.reps, "warmup": args.warmup})
                lines.append(info)
                print(json.dumps(info), flush=True)
            cond = [x for x in lines if x["is_condition"]]
            verdict = {"driver_condition_met": bool(all(x["device_within_host_iqr"] for x in cond))}
            lines.append(verdict)
            print(json.dumps(verdict), flush=True)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
