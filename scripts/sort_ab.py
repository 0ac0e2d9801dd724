#!/usr/bin/env python3
"""What the device sort of a resident methylome costs (abn_sites_sort), and what the alternatives cost.

Per shape — one sample of 2 M records (a CG-sized methylome) and one of 30 M (CHH-sized) — and per input — its lines
shuffled, already in canonical order, and sorted by (chromosome, strand, start) — on one device:

  1. medians of 7 calls of abn_sites_sort_info's four times (flatten, check, the sort passes, gather), and the passes run;
  2. next to them, on the same records: the serial host form (abn_sites_sort_keys_host) on this machine's CPU, and the
     device parse of the text the records came from (abn_sites_parse_dev: kernel_ms and wall time with the upload);
  3. from the design: a pass reads and writes every 16-byte (key, index) pair once, 32 B per record and pass; the measured
     pass time against that byte count at the HBM rate (--hbm-gbs), as a ratio, nothing promised.

The texts are built with numpy as fixed-width lines (zero-padded positions, which the parser reads as it reads any digits),
all CG, five chromosomes.  Writes one JSON document (--out) and prints it.
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


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    q1, med, q3 = np.percentile(xs, [25, 50, 75])
    return {"median": float(med), "iqr": float(q3 - q1), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def rows_of(chromosome, start, strand):
    """the fixed-width lines of the records, a uint8 matrix (n, len(ROW))"""
    n = len(chromosome)
    rows = np.tile(np.frombuffer(ROW, dtype=np.uint8), (n, 1))
    rows[:, 0] = ord("0") + chromosome
    rest = start.astype(np.int64)
    for col in range(10, 1, -1):
        rows[:, col] = ord("0") + rest % 10
        rest //= 10
    rows[:, 12] = np.where(strand == 0, ord("+"), ord("-"))
    return rows


def records(n, kind, seed):
    """(chromosome, start, strand) of n records on five chromosomes, a site every 3 bp on alternating strands"""
    i = np.arange(n, dtype=np.int64)
    per = (n + 4) // 5
    chromosome, within = 1 + i // per, i % per
    start, strand = 3 * within + 1, within % 2
    if kind == "shuffled":
        order = np.random.default_rng(seed).permutation(n)
    elif kind == "by_strand":
        order = np.lexsort((start, strand, chromosome))
    else:
        order = i
    return chromosome[order], start[order], strand[order]


def measure(abn, ctx, n, kind, reps, host_reps, parse_reps, hbm_gbs):
    chromosome, start, strand = records(n, kind, seed=n)
    text = HEADER + rows_of(chromosome, start, strand).tobytes()
    out = {"records": n, "input": kind, "text_bytes": len(text)}
    wall, kernel = [], []
    parent = None
    for _ in range(parse_reps):
        if parent is not None:
            parent.close()
        t0 = time.perf_counter()
        parent = ctx.parse_sites_resident(text, skip_lines=1)
        wall.append(1e3 * (time.perf_counter() - t0))
        kernel.append(parent.info()["kernel_ms"])
    assert parent.info()["n_sites"] == n and parent.info()["n_deferred"] == 0
    out["device_parse"] = {"kernel_ms": stats(kernel), "wall_ms_with_upload": stats(wall)}
    del text
    ms = []
    for _ in range(reps + 1):                                                # the first call is a warm-up
        child = parent.sort()
        info = child.sort_info()
        ms.append(info["ms"].copy())
        child.close()
    parent.close()
    ms = np.array(ms[1:])
    out["passes"], out["descents"] = info["passes"], info["descents"]
    out["sort_ms"] = {name: stats(ms[:, k]) for k, name in enumerate(("flatten", "check", "passes", "gather"))}
    out["sort_ms"]["total"] = stats(ms.sum(axis=1))
    if info["passes"]:
        per_pass = out["sort_ms"]["passes"]["median"] / info["passes"]
        floor = 32.0 * n / (hbm_gbs * 1e9) * 1e3
        out["pass_model"] = {"bytes_per_record_and_pass": 32, "ms_per_pass": per_pass, "ms_at_hbm_rate": floor,
                             "hbm_gbs": hbm_gbs, "ratio": per_pass / floor}
    end = (start + 1).astype(np.uint32)
    host = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        order, hinfo = abn.sort_sites_host(chromosome, start, end, strand)
        host.append(1e3 * (time.perf_counter() - t0))
    assert hinfo["passes"] == info["passes"] and hinfo["descents"] == info["descents"]
    out["host_serial_ms"] = stats(host)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--shapes", default="2000000,30000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM rate the pass model divides by [GB/s]")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sort_ab.json"))
    args = ap.parse_args()
    import alphabeta_rs_amd as abn

    ctx = abn.Context(args.device)
    doc = {"what": "abn_sites_sort: medians of HIP-event ms over --reps calls; serial host form; device parse of the same text",
           "reps": args.reps, "runs": []}
    try:
        for n in (int(s) for s in args.shapes.split(",")):
            big = n > 5_000_000
            for kind in ("shuffled", "sorted", "by_strand"):
                run = measure(abn, ctx, n, kind, args.reps, host_reps=1 if big else 3, parse_reps=2 if big else 3,
                              hbm_gbs=args.hbm_gbs)
                doc["runs"].append(run)
                print(json.dumps(run), flush=True)
    finally:
        ctx.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
