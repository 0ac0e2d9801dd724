#!/usr/bin/env python3
"""What genomic tiles cost (abn_tiles_*, csrc/abn_tiles.hpp), on --samples (8) methylomes of --sites (2 000 000) CG rows on
five chromosomes of --span (20 000 000) bp, the later samples' statuses drifting from the first's:

  kernels  per tile size (100 kb; 2 kb for many short jobs): the HIP-event times of the tile search and the tile fold
           (Tiles.kernel_ms after set_fixed), the host clock around set_fixed, and the HIP-event time of the windows-packed
           scan over the tiles' column ranges (pairwise_divergence_windows_packed_dev on the same matrix), --warmup runs
           dropped, the median of --reps;
  baseline the existing whole-sample fold on the same sites, abn_codes_fold_kernel (Codes.kernel_ms()[3]), alternating with
           the tile folds in one process: n chains where the tile fold has n x T;
  wall     `metaprofile_alphabeta --tiles 100000` next to one `alphabeta --sites device` run on the same files (host
           clock around the process, --wall-reps each, alternating; --iterations fits per tile and for the one pedigree).

Before anything is timed the tile folds are checked against the whole-sample fold where they must agree: the kept counts of
the tiles of one step sum to the sample's.  Prints one JSON line and writes it to --out (default profiles/tiles_ab.json).
"""
import argparse
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

import genes_ab  # noqa: E402  (its statistics)

HEADER = genes_ab.HEADER
CHROMOSOMES = 5
# two lineages from one founder: 8 sampled nodes
NODES = [("0_0", 0, True), ("1_2", 1, True), ("2_2", 2, True), ("3_2", 3, False), ("4_2", 4, True),
         ("1_8", 1, True), ("2_8", 2, True), ("3_8", 3, True), ("4_8", 4, True)]
EDGES = [("0_0", "1_2"), ("1_2", "2_2"), ("2_2", "3_2"), ("3_2", "4_2"), ("0_0", "1_8"), ("1_8", "2_8"), ("2_8", "3_8"),
         ("3_8", "4_8")]


def methylomes(n_samples, n_sites, span, seed):
    """CG rows, the chromosomes one after the other, starts strictly ascending inside each; sample k's statuses are sample
    k - 1's with 2 % redrawn, its levels follow its statuses"""
    rng = np.random.default_rng(seed)
    per = n_sites // CHROMOSOMES
    chrom = np.repeat(np.arange(1, CHROMOSOMES + 1), per).astype(str)
    pos = np.concatenate([np.sort(rng.choice(span, size=per, replace=False)) + 1 for _ in range(CHROMOSOMES)]).astype(str)
    n = len(pos)
    strand = np.where(rng.integers(0, 2, size=n) == 0, "+", "-")
    status = rng.choice([0, 2], size=n, p=[0.6, 0.4])
    texts = []
    for k in range(n_samples):
        if k:
            status = np.where(rng.random(n) < 0.02, rng.integers(0, 3, size=n), status)
        pm = np.char.mod("%.4f", np.where(rng.random(n) < 0.9, 0.99 + 0.0099 * rng.random(n), rng.random(n)))
        lvl = np.char.mod("%.4f", 0.05 + 0.45 * status + 0.04 * rng.random(n))
        st = np.array(list("UIM"))[status]
        cols = chrom, pos, strand, ["CG"] * n, ["3"] * n, ["8"] * n, pm, st, lvl, ["CGA"] * n
        texts.append((HEADER + "\n".join("\t".join(r) for r in zip(*cols)) + "\n").encode())
    return texts


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--span", type=int, default=20_000_000)
    ap.add_argument("--tile-sizes", type=int, nargs="+", default=[100_000, 2_000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--wall-reps", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "tiles_ab.json")
    args = ap.parse_args()
    if args.samples > len([n for n in NODES if n[2]]):
        ap.error("at most 8 samples: the pedigree of the wall-time runs has 8 sampled nodes")
    import alphabeta_rs_amd as A
    from alphabeta_rs_amd import build as B

    A.load_library(build_if_missing=True)
    B.build_host()
    if A.device_count() <= 0:
        sys.exit("no HIP device: every number here is a device time, nothing to measure")
    stats = genes_ab.stats
    texts = methylomes(args.samples, args.sites, args.span, 11)
    result = {"samples": args.samples, "sites_per_sample": args.sites // CHROMOSOMES * CHROMOSOMES, "span": args.span,
              "reps": args.reps, "warmup": args.warmup, "text_bytes": int(sum(map(len, texts))), "tiles": {}}
    with A.Context(0) as ctx:
        sites = []
        for t in texts:
            r = ctx.parse_sites_resident(t, skip_lines=0)
            assert r.info()["n_deferred"] == 0                   # four-decimal values: the device is certain of every line
            sites.append(r)
        codes = A.Codes.from_parsed(ctx, sites, posterior_max_filter=0.99)
        tiles = A.Tiles.from_parsed(ctx, sites, posterior_max_filter=0.99)
        assert tiles.n_columns == codes.n_sites == result["sites_per_sample"] and tiles.n_runs == CHROMOSOMES
        whole_kept = codes.stats()[2]
        folds = {"whole_sample": []}
        for size in args.tile_sizes:
            tiles.set_fixed(size)
            count, _, kept = tiles.stats()
            assert kept.sum(axis=1).tolist() == whole_kept.tolist() and count.sum() == tiles.n_columns
            begin, end = tiles.layout()
            search, fold, scan, clock = [], [], [], []
            for rep in range(args.warmup + args.reps):
                again = A.Codes.from_parsed(ctx, sites, posterior_max_filter=0.99)      # the whole-sample fold, alternating
                whole = again.kernel_ms()[3]
                again.close()
                t0 = time.perf_counter()
                tiles.set_fixed(size)
                t1 = time.perf_counter()
                ms = tiles.kernel_ms()
                scan_ms = ctx.pairwise_divergence_windows_packed_dev(codes.packed_device_ptr(), args.samples, codes.n_sites,
                                                                     codes.row_stride, begin, end)
                if rep >= args.warmup:
                    folds["whole_sample"].append(whole)
                    search.append(ms[0]), fold.append(ms[1]), scan.append(scan_ms), clock.append(t1 - t0)
            result["tiles"][str(size)] = {"n_tiles": int(len(begin)), "fold_jobs": int(len(begin)) * args.samples,
                                          "columns_per_tile_median": float(np.median(count)), "columns_per_tile_max": int(count.max()),
                                          "search_ms": stats(search), "fold_ms": stats(fold), "scan_ms": stats(scan),
                                          "set_fixed_s": stats(clock)}
            print(json.dumps({size: result["tiles"][str(size)]}), file=sys.stderr, flush=True)
        result["whole_sample_fold_ms"] = stats(folds["whole_sample"])
        tiles.close()
        codes.close()
        for s in sites:
            s.close()
    # the wall time of the two tools on the same files
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        meth = tmp / "methylome"
        meth.mkdir()
        sampled = [n for n in NODES if n[2]][:args.samples]
        for (name, _, _), t in zip(sampled, texts):
            (meth / f"G{name}.txt").write_bytes(t)
        keep = {n[0] for n in sampled}
        (tmp / "nodelist.fn").write_text("filename\tnode\tgen\tmeth\n" + "".join(
            (f"{meth}/G{name}.txt" if name in keep else "-") + f"\t{name}\t{gen}\t{'Y' if name in keep else 'N'}\n"
            for name, gen, _ in NODES))
        (tmp / "edgelist.fn").write_text("from\tto\tgendiff\n" + "".join(f"{a}\t{b}\t1\n" for a, b in EDGES))
        wall = {"tiles": [], "alphabeta": []}
        lines = 0
        for rep in range(1 + args.wall_reps):                      # the first pair warms the file cache and is dropped
            for side in ("tiles", "alphabeta"):
                out = tmp / f"out_{side}_{rep}"
                out.mkdir()
                graph = ["--nodes", tmp / "nodelist.fn", "--edges", tmp / "edgelist.fn"]
                cmd = [B.META_CLI, "-o", out, "--methylome", meth, *graph, "--tiles", args.tile_sizes[0], "--iterations",
                       args.iterations] if side == "tiles" else \
                    [B.CLI, "-i", args.iterations, "-n", tmp / "nodelist.fn", "-e", tmp / "edgelist.fn", "-o", out, "--parse",
                     "device", "--sites", "device"]
                t0 = time.perf_counter()
                r = subprocess.run(list(map(str, cmd)), capture_output=True, text=True, timeout=900)
                t1 = time.perf_counter()
                if r.returncode != 0:
                    sys.exit(f"{side}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                if side == "tiles":
                    lines = len((out / "results.txt").read_text().splitlines()) - 1
                if rep:
                    wall[side].append(t1 - t0)
        result["wall"] = {"iterations": args.iterations, "tile_size": args.tile_sizes[0], "tiles_fitted": lines,
                          "metaprofile_tiles_s": stats(wall["tiles"]), "alphabeta_sites_device_s": stats(wall["alphabeta"])}
    print(json.dumps(result), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
