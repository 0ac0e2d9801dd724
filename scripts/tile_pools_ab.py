#!/usr/bin/env python3
"""What region pools cost (abn_tiles_set_pools, csrc/abn_tiles.hpp: pools), on the inputs of scripts/tiles_ab.py: --samples
(8) methylomes of --sites (2 000 000) CG rows on five chromosomes of --span (20 000 000) bp, and --intervals (30 000) short
intervals (100 .. 500 bp, anywhere on the five chromosomes) in --pools (4) pools.  Two ways to the same pooled pedigrees,
alternating in one process, --warmup runs dropped, the median of --reps:

  pools   Tiles.set_pools on the resident, aligned methylomes: the HIP-event times of search, offsets, map, gather, pack and
          fold (kernel_ms, pool_kernel_ms), the host clock around the call, and around Tiles.pairwise();
          the scan's own kernel time is taken on a Codes matrix built from the pooled lines of all pools side by side, which
          is the pooled matrix (the same kernel, the same ranges);
  detour  what the handle offered before: every methylome's text cut down to a pool's lines on the host (host clock, timed
          apart), then per pool parse_sites_resident of the 8 cut texts, Codes.from_parsed and Codes.pairwise (host clock
          around each; Codes.kernel_ms beside them).

Before anything is timed the two are compared: every pool's count, kept, level_sum_kept bits and pairwise arrays.  Prints one
JSON line and writes it to --out (default profiles/tile_pools_ab.json)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

import genes_ab  # noqa: E402  (its statistics)
import tiles_ab  # noqa: E402  (its methylomes)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--span", type=int, default=20_000_000)
    ap.add_argument("--intervals", type=int, default=30_000)
    ap.add_argument("--pools", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "tile_pools_ab.json")
    args = ap.parse_args()
    import alphabeta_rs_amd as A

    A.load_library(build_if_missing=True)
    if A.device_count() <= 0:
        sys.exit("no HIP device: every number here is a device time, nothing to measure")
    stats = genes_ab.stats
    n, P = args.samples, args.pools
    texts = tiles_ab.methylomes(n, args.sites, args.span, 11)
    rng = np.random.default_rng(12)
    chrom = rng.integers(1, tiles_ab.CHROMOSOMES + 1, size=args.intervals).astype(np.int32)
    lo = rng.integers(0, args.span, size=args.intervals).astype(np.int64)
    hi = lo + rng.integers(100, 501, size=args.intervals)
    pool = rng.integers(0, P, size=args.intervals).astype(np.int32)
    result = {"samples": n, "sites_per_sample": args.sites // tiles_ab.CHROMOSOMES * tiles_ab.CHROMOSOMES, "span": args.span,
              "intervals": args.intervals, "pools": P, "reps": args.reps, "warmup": args.warmup}
    with A.Context(0) as ctx:
        sites = []
        for t in texts:
            r = ctx.parse_sites_resident(t, skip_lines=0)
            assert r.info()["n_deferred"] == 0
            sites.append(r)
        tiles = A.Tiles.from_parsed(ctx, sites, posterior_max_filter=0.99)
        tiles.set_pools(chrom, lo, hi, pool, P)
        begin, end = tiles.layout()
        src = tiles.pool_columns()
        count, lsk, kept = tiles.stats()
        pairs = tiles.pairwise()
        result.update({"segments": int(len(tiles.pool_segments()[0])), "pooled_columns": int(len(src)),
                       "columns_per_pool": count.tolist()})
        # the detour's inputs: every text cut down to a pool's lines on the host (align none: column k is line k)
        t0 = time.perf_counter()
        lines = [np.array(t.split(b"\n")[1:-1], dtype=object) for t in texts]
        header = tiles_ab.HEADER.encode()
        cut = [[header + b"\n".join(lines[s][src[begin[p]:end[p]]].tolist()) + b"\n" for s in range(n)] for p in range(P)]
        result["host_filter_s"] = time.perf_counter() - t0
        result["cut_text_bytes"] = int(sum(len(t) for per in cut for t in per))

        def detour(check):
            """-> host-clock seconds of (parse, build, pairwise) and the kernel ms of the builds, summed over the pools"""
            spent, kernel = np.zeros(3), 0.0
            for p in range(P):
                t0 = time.perf_counter()
                small = [ctx.parse_sites_resident(t, skip_lines=0) for t in cut[p]]
                t1 = time.perf_counter()
                codes = A.Codes.from_parsed(ctx, small, posterior_max_filter=0.99)
                t2 = time.perf_counter()
                got = codes.pairwise()
                t3 = time.perf_counter()
                spent += (t1 - t0, t2 - t1, t3 - t2)
                kernel += float(codes.kernel_ms().sum())
                if check:
                    c, s, k = codes.stats()
                    assert c.tolist() == [count[p]] * n and k.tolist() == kept[:, p].tolist()
                    assert s.tobytes() == np.ascontiguousarray(lsk[:, p]).tobytes()
                    for g, w in zip(pairs, got):
                        assert g[p].tobytes() == w.tobytes()
                codes.close()
                for x in small:
                    x.close()
            return spent, kernel

        detour(check=True)
        # the pooled matrix once more as a Codes matrix, for the scan's kernel time
        side = [ctx.parse_sites_resident(header + b"\n".join(lines[s][src].tolist()) + b"\n", skip_lines=0) for s in range(n)]
        whole = A.Codes.from_parsed(ctx, side, posterior_max_filter=0.99)
        assert whole.n_sites == len(src)
        keys = ("search", "fold", "offsets", "map", "gather", "pack")
        kernel = {k: [] for k in keys + ("scan",)}
        wall = {"set_pools_s": [], "pairwise_s": [], "detour_parse_s": [], "detour_build_s": [], "detour_pairwise_s": []}
        detour_kernel = []
        for rep in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            tiles.set_pools(chrom, lo, hi, pool, P)
            t1 = time.perf_counter()
            tiles.pairwise()
            t2 = time.perf_counter()
            ms = np.concatenate([tiles.kernel_ms(), tiles.pool_kernel_ms()])
            scan_ms = ctx.pairwise_divergence_windows_packed_dev(whole.packed_device_ptr(), n, whole.n_sites, whole.row_stride,
                                                                 begin, end)
            spent, dk = detour(check=False)
            if rep >= args.warmup:
                for k, v in zip(keys, ms):
                    kernel[k].append(float(v))
                kernel["scan"].append(float(scan_ms))
                wall["set_pools_s"].append(t1 - t0), wall["pairwise_s"].append(t2 - t1)
                wall["detour_parse_s"].append(spent[0]), wall["detour_build_s"].append(spent[1])
                wall["detour_pairwise_s"].append(spent[2])
                detour_kernel.append(dk)
        result["kernel_ms"] = {k: stats(v) for k, v in kernel.items()}
        result["wall"] = {k: stats(v) for k, v in wall.items()}
        result["detour_build_kernel_ms"] = stats(detour_kernel)
        pools_s = np.array(wall["set_pools_s"]) + np.array(wall["pairwise_s"])
        detour_s = np.array(wall["detour_parse_s"]) + np.array(wall["detour_build_s"]) + np.array(wall["detour_pairwise_s"])
        result["pools_total_s"], result["detour_total_s"] = stats(pools_s.tolist()), stats(detour_s.tolist())
        result["detour_over_pools"] = float(np.median(detour_s) / np.median(pools_s))
        result["detour_with_filter_over_pools"] = float((np.median(detour_s) + result["host_filter_s"]) / np.median(pools_s))
        whole.close()
        for x in side:
            x.close()
        tiles.close()
        for s in sites:
            s.close()
    print(json.dumps(result), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
