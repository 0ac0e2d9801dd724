#!/usr/bin/env python3
"""What the collapse of a resident methylome's repeated sites costs on the device (abn_sites_dedup), and its yardsticks.

Per shape — one sample of 2 M records (a CG-sized methylome) and one of 30 M (CHH-sized), in canonical order — and per
repeat pattern — no repeats, every hundredth key doubled (1 %), every key doubled, and runs of 8 (under `best` only) — on one
device:

  1. per policy, medians of 7 calls of abn_sites_dedup_info's four times (flatten, flags with BEST's walk, scan, gather);
  2. next to them, on the same records and in the same process: abn_sites_sort of the same in-order input (its four times;
     it runs no pass) and the serial host form of the collapse (abn_sites_dedup_keys_host) on this machine's CPU;
  3. the ratios collapse / in-order sort and serial host form / collapse, nothing promised.  By byte count the collapse is
     that sort without a pass, plus one flag byte per record and one scan.

The texts are built with numpy as fixed-width lines, all CG, five chromosomes; the last digit of posteriormax and the
status vary along the records, so the repeats disagree.  Writes one JSON document (--out) and prints its rows.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
HEADER = (b"seqnames\tstart\tstrand\tcontext\tcounts.methylated\tcounts.total\tposteriorMax\tstatus\trc.meth.lvl\t"
          b"context.trinucleotide\n")
ROW = b"1\t000000000\t+\tCG\t3\t8\t0.9999\tM\t0.5000\n"
POLICIES = ("first", "last", "best", "drop")
PATTERNS = {"none": (1, 0), "1 %": (2, 100), "doubled": (2, 1), "runs of 8": (8, 1)}   # (run length, of every k-th key)


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    q1, med, q3 = np.percentile(xs, [25, 50, 75])
    return {"median": float(med), "iqr": float(q3 - q1), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def records(n, pattern):
    """(chromosome, start, strand, posterior digit, status) of n records in canonical order on five chromosomes, a key every
    3 bp on alternating strands, the keys repeated as the pattern says"""
    length, every = PATTERNS[pattern]
    if every == 0:
        key = np.arange(n, dtype=np.int64)
    else:
        m = n if every > 1 else (n + length - 1) // length
        lengths = np.where(np.arange(m) % every == 0, length, 1)
        key = np.repeat(np.arange(m, dtype=np.int64), lengths)[:n]
    per = (int(key[-1]) + 5) // 5
    chromosome, within = 1 + key // per, key % per
    i = np.arange(n, dtype=np.int64)
    return chromosome, 3 * within + 1, within % 2, (i * 7) % 10, i % 3


def text_of(chromosome, start, strand, digit, status):
    n = len(chromosome)
    rows = np.tile(np.frombuffer(ROW, dtype=np.uint8), (n, 1))
    rows[:, 0] = ord("0") + chromosome
    rest = start.astype(np.int64)
    for col in range(10, 1, -1):
        rows[:, col] = ord("0") + rest % 10
        rest //= 10
    rows[:, 12] = np.where(strand == 0, ord("+"), ord("-"))
    rows[:, 26] = ord("0") + digit
    rows[:, 28] = np.frombuffer(b"UIM", dtype=np.uint8)[status % 3]
    return HEADER + rows.tobytes()


def measure(dedup, ctx, n, pattern, policies, reps, host_reps):
    chromosome, start, strand, digit, status = records(n, pattern)
    parent = ctx.parse_sites_resident(text_of(chromosome, start, strand, digit, status), skip_lines=1)
    assert parent.info()["n_sites"] == n and parent.info()["n_deferred"] == 0
    rows = []
    try:
        ms = []
        for _ in range(reps + 1):                                            # the first call is a warm-up
            child = parent.sort()
            info = child.sort_info()
            ms.append(info["ms"].copy())
            child.close()
        assert info["descents"] == 0 and info["passes"] == 0
        sort_total = stats(np.array(ms[1:]).sum(axis=1))
        f = parent.fetch()
        for policy in policies:
            ms = []
            for _ in range(reps + 1):
                child = dedup.dedup(parent, policy)
                info = dedup.dedup_info(child)
                ms.append(info["ms"].copy())
                child.close()
            ms = np.array(ms[1:])
            row = {"records": n, "repeats": pattern, "policy": policy, "kept": info["kept"], "repeated": info["repeated"],
                   "disagreeing": info["disagreeing"],
                   "dedup_ms": {name: stats(ms[:, k]) for k, name in enumerate(("flatten", "flags", "scan", "gather"))},
                   "in_order_sort_ms": sort_total}
            row["dedup_ms"]["total"] = stats(ms.sum(axis=1))
            host = []
            for _ in range(host_reps):
                t0 = time.perf_counter()
                order, hinfo = dedup.dedup_sites_host(f["chromosome"], f["start"], f["end"], f["strand"], f["posteriormax"],
                                                    f["status"], policy=policy)
                host.append(1e3 * (time.perf_counter() - t0))
            assert hinfo == {k: info[k] for k in hinfo}
            row["host_serial_ms"] = stats(host)
            row["ratio_to_in_order_sort"] = row["dedup_ms"]["total"]["median"] / sort_total["median"]
            row["host_serial_over_device"] = row["host_serial_ms"]["median"] / row["dedup_ms"]["total"]["median"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        parent.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--shapes", default="2000000,30000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dedup_ab.json"))
    args = ap.parse_args()
    import alphabeta_rs_amd as abn
    from alphabeta_rs_amd import dedup

    ctx = abn.Context(args.device)
    doc = {"what": "abn_sites_dedup: medians of HIP-event ms over --reps calls; abn_sites_sort of the same in-order input; "
                   "serial host form", "reps": args.reps, "runs": []}
    try:
        for n in (int(s) for s in args.shapes.split(",")):
            for pattern in PATTERNS:
                policies = ("best",) if pattern == "runs of 8" else POLICIES
                doc["runs"] += measure(dedup, ctx, n, pattern, policies, args.reps, host_reps=1 if n > 5_000_000 else 3)
    finally:
        ctx.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
