#!/usr/bin/env python3
"""The segment table of the one-window step (docs/experiments.md, "Early bootstraps") from a rocprofv3 kernel trace
(`*_kernel_trace.csv`) of scripts/step_chain_run.py or of bench.py's default workload.

    python scripts/step_chain_table.py TRACE.csv [--skip 3] [--json OUT.json]

A step is cut at the clear that directly precedes pass 1 of phase A (the only speculative launch that follows a clear on
its queue); everything dispatched before the next such clear belongs to it.  Segments, in microseconds, median over the steps:
  (a) first dispatch of the step (its first clear) -> end of pass 1 of phase A
  (b) end of pass 1 -> start of phase B (the persistent kernel's first launch)
  (c) start of phase B -> end of its tail's resume launch (the first speculative launch behind it)
  (d) end of that launch -> end of the step's last dispatch
and whether the stragglers' resume launch (the speculative launch between pass 1 and phase B's end that is not on phase
A's queue position) overlaps phase B in time."""
from __future__ import annotations

import argparse
import csv
import json
import statistics


def short(name: str) -> str:
    for key in ("abn_fit_spec_kernel", "abn_fit_refill_kernel", "abn_fit_kernel", "abn_select_lse_kernel", "abn_select_kernel",
                "abn_early_compare_kernel", "abn_early_adopt_kernel", "abn_step_prepare_kernel", "fillBuffer", "copyBuffer"):
        if key in name:
            return key
    return name.split("(")[0][-40:]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--skip", type=int, default=3, help="leading steps left out (warm-up)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--list", action="store_true", help="print the dispatches of the first kept step")
    args = ap.parse_args()

    rows = []
    with open(args.trace, newline="") as f:
        for r in csv.DictReader(f):
            rows.append({"name": short(r["Kernel_Name"]), "t0": int(r["Start_Timestamp"]), "t1": int(r["End_Timestamp"]),
                         "grid": int(r["Grid_Size_X"]), "queue": r["Queue_Id"], "stream": r.get("Stream_Id", "")})
    rows.sort(key=lambda r: r["t0"])
    # A step's head is the clear (fill kernels, or the preparation launch) that directly precedes pass 1 of phase A on its
    # queue: no other speculative launch follows a clear (the stragglers' follows the fork, the tails' a persistent launch).
    CLEARS = ("fillBuffer", "abn_step_prepare_kernel")
    steps = []
    for j, r in enumerate(rows):
        if r["name"] != "abn_fit_spec_kernel":
            continue
        prev = next((i for i in range(j - 1, -1, -1) if rows[i]["queue"] == r["queue"]), None)
        if prev is None or rows[prev]["name"] not in CLEARS:
            continue
        head = prev
        while head - 1 >= 0 and rows[head - 1]["name"] in CLEARS and rows[head - 1]["queue"] == r["queue"]:
            head -= 1
        steps.append({"head": head, "a": j})
    for k in range(len(steps) - 1):
        steps[k]["last"] = steps[k + 1]["head"] - 1
    steps = steps[:-1]    # the last step has no successor to bound it
    for s in steps:       # phase B: the step's first persistent launch (a redo would be the second)
        s["b"] = next((i for i in range(s["a"], s["last"] + 1) if rows[i]["name"] == "abn_fit_refill_kernel"), None)
    steps = [s for s in steps if s["b"] is not None][args.skip:]
    if not steps:
        raise SystemExit("no complete steps (is phase B on the persistent kernel?)")

    seg = {"a": [], "b": [], "c": [], "d": [], "step": [], "pass1": [], "phaseB": [], "dispatches": []}
    overlap = []
    for s in steps:
        ra, rb = rows[s["a"]], rows[s["b"]]
        within = rows[s["head"]:s["last"] + 1]
        # phase B's tail resume: the first speculative launch on phase B's queue that starts at or after phase B's end
        tail = next((r for r in within if r["name"] == "abn_fit_spec_kernel" and r["t0"] >= rb["t1"] - 1000 and r is not ra), None)
        tail_end = tail["t1"] if tail else rb["t1"]
        end = max(r["t1"] for r in within)
        seg["a"].append((ra["t1"] - rows[s["head"]]["t0"]) / 1e3)
        seg["b"].append((rb["t0"] - ra["t1"]) / 1e3)
        seg["c"].append((tail_end - rb["t0"]) / 1e3)
        seg["d"].append((end - tail_end) / 1e3)
        seg["step"].append((end - rows[s["head"]]["t0"]) / 1e3)
        seg["pass1"].append((ra["t1"] - ra["t0"]) / 1e3)
        seg["phaseB"].append((rb["t1"] - rb["t0"]) / 1e3)
        seg["dispatches"].append(len(within))
        strag = [r for r in within if r["name"] == "abn_fit_spec_kernel" and r is not ra and r is not tail and r["t0"] < rb["t1"]
                 and r["t0"] >= ra["t1"]]
        if strag:
            r = strag[0]
            overlap.append({"straggler_us": (r["t1"] - r["t0"]) / 1e3, "starts_after_pass1_us": (r["t0"] - ra["t1"]) / 1e3,
                            "ends_after_phaseB_start_us": (r["t1"] - rb["t0"]) / 1e3,
                            "overlaps": r["t1"] > rb["t0"] and r["t0"] < rb["t1"], "queue": r["queue"], "main_queue": rb["queue"]})
    if args.list:
        s = steps[0]
        t0 = rows[s["head"]]["t0"]
        for r in rows[s["head"]:s["last"] + 1]:
            print(f"{(r['t0'] - t0) / 1e3:10.2f} {(r['t1'] - t0) / 1e3:10.2f} {(r['t1'] - r['t0']) / 1e3:9.2f} us  q{r['queue']} s{r['stream']}"
                  f"  grid {r['grid']:7d}  {r['name']}")
    med = {k: statistics.median(v) for k, v in seg.items()}
    out = {"trace": args.trace, "steps": len(steps), "median_us": med,
           "min_us": {k: min(v) for k, v in seg.items()}, "max_us": {k: max(v) for k, v in seg.items()}}
    if overlap:
        out["stragglers"] = {"steps_overlapping_phase_b": sum(1 for o in overlap if o["overlaps"]), "of": len(overlap),
                             "median_straggler_us": statistics.median(o["straggler_us"] for o in overlap),
                             "median_start_after_pass1_us": statistics.median(o["starts_after_pass1_us"] for o in overlap),
                             "median_end_after_phase_b_start_us": statistics.median(o["ends_after_phaseB_start_us"] for o in overlap),
                             "queues": sorted({(o["queue"], o["main_queue"]) for o in overlap})}
    print(json.dumps(out, indent=1))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
