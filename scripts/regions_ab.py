#!/usr/bin/env python3
"""What region-level states cost (abn_packed_region_states_dev, csrc/abn_regions.hpp), on a packed matrix of the tiles
benchmark's size (scripts/tiles_ab.py, profiles/tiles_ab.json: --samples 8 rows of --sites 2 000 000 sites), cut into
contiguous tiles of --tile-sites 8, 16, 64, 256, 1024 and 4096 sites:

  fused    the HIP-event time of abn_region_states_kernel with every tile walked by its lane (long_sites above the tile);
  census   the HIP-event time of abn_packed_census_windows_dev over the same windows — the route that existed before, one
           256-lane workgroup per (tile, sample), and the only baseline: it gives the counts the rule is then a few
           integer operations of;
  routed   the fused entry with long_sites = the tile (every window through the census, then the kernel reading the table):
           what the long-window route costs in all.

The sides alternate in one process, --warmup runs dropped, the median and spread of --reps.  Before anything is timed
the fused result is held to the host's serial form on the first 4 096 windows, and both routes to each other on all.  Two
crossovers are reported, each the first tile length of the list at which the walked kernel is no faster: than the census
kernels alone (census_crossover_tile_sites, what kRegionLongSites is set from) and than the routed entry
(crossover_tile_sites).  Every tile length runs in
a child process of its own under a time limit; the first that fails ends the run.  Prints one JSON line and writes it to
--out (default profiles/regions_ab.json).
"""
import argparse
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

RULE = (250_000, 750_000, 1_000_000, 1)


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    q1, med, q3 = np.percentile(xs, [25, 50, 75])
    return {"median": float(med), "iqr": float(q3 - q1), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def packed_matrix(n, sites, seed):
    """random fields (U 0.5, I 0.1, M 0.3, filtered 0.1) in the packed format: site 16 g + 4 j + e in byte 4 g + e, bits 2j.."""
    rng = np.random.default_rng(seed)
    stride = (sites + 255) // 256 * 64
    f = np.full((n, 4 * stride), 3, dtype=np.uint8)
    f[:, :sites] = rng.choice(4, size=(n, sites), p=[0.5, 0.1, 0.3, 0.1])
    f = f.reshape(n, stride // 4, 4, 4)                                   # [row][g][j][e]
    return (f[:, :, 0, :] | f[:, :, 1, :] << 2 | f[:, :, 2, :] << 4 | f[:, :, 3, :] << 6).reshape(n, stride).astype(np.uint8)


def out_stride(columns):
    """abn_packed_row_stride"""
    return 0 if columns <= 0 else (columns + 255) // 256 * 64


def hip_runtime():
    h = C.CDLL("libamdhip64.so")
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def measure(args, tile):
    import alphabeta_rs_amd as A
    from alphabeta_rs_amd import census, regions

    A.load_library(build_if_missing=True)
    if A.device_count() <= 0:
        sys.exit("no HIP device: every number here is a device time, nothing to measure")
    n, sites = args.samples, args.sites
    packed = packed_matrix(n, sites, 11)
    begin = np.arange(0, sites, tile, dtype=np.int64)
    end = np.minimum(begin + tile, sites)
    T = len(begin)
    out_bytes = n * out_stride(T)
    hip = hip_runtime()
    bufs = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
    sizes = [packed.nbytes, out_bytes, T * n * 3 * 8]
    for b, size in zip(bufs, sizes):
        if hip.hipMalloc(C.byref(b), size) != 0:
            sys.exit("hipMalloc failed")
    try:
        assert hip.hipMemcpy(bufs[0], packed.ctypes.data, packed.nbytes, 1) == 0
        walked_ls = (tile // 16 + 1) * 16                                # above the tile: every window walked by its lane
        routed_ls = tile // 16 * 16                                      # at most the tile: every window through the census
        # (long_sites is a multiple of 16: tiles below 16 sites cannot be routed, and have no third column)
        with A.Context(0) as ctx:
            def fused(long_sites):
                return regions.region_states_dev(ctx, bufs[0].value, n, sites, packed.shape[1], begin, end, *RULE, bufs[1].value,
                                                 long_sites=long_sites)

            def fetch():
                got = np.zeros((n, out_stride(T)), dtype=np.uint8)
                assert hip.hipMemcpy(got.ctypes.data, bufs[1], got.nbytes, 2) == 0
                return got

            fused(walked_ls)
            walked = fetch()
            head = min(T, 4096)
            want = regions.region_states_host(packed, sites, begin[:head], end[:head], *RULE)
            assert walked[:, :head // 16 * 4].tobytes() == want[:, :head // 16 * 4].tobytes(), "the kernel differs from the law"
            if routed_ls:
                fused(routed_ls)
                assert fetch().tobytes() == walked.tobytes(), "the two routes differ"
            t_fused, t_census, t_routed = [], [], []
            for rep in range(args.warmup + args.reps):
                a = fused(walked_ls)
                b = census.census_windows_dev(ctx, bufs[0].value, n, sites, packed.shape[1], begin, end, bufs[2].value)
                c = fused(routed_ls) if routed_ls else [np.nan, np.nan]
                if rep >= args.warmup:
                    t_fused.append(a[1]), t_census.append(b), t_routed.append(c[0] + c[1])
        return {"tile_sites": tile, "windows": T, "fused_ms": stats(t_fused), "census_ms": stats(t_census),
                "routed_ms": stats(t_routed) if routed_ls else None,
                "census_over_fused": float(np.median(t_census) / np.median(t_fused)),
                "routed_over_fused": float(np.median(t_routed) / np.median(t_fused)) if routed_ls else None}
    finally:
        for b in bufs:
            hip.hipFree(b)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--tile-sites", type=int, nargs="+", default=[8, 16, 64, 256, 1024, 4096])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per tile length")
    ap.add_argument("--one", type=int, default=0, help="(internal) measure this tile length and print its JSON")
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "regions_ab.json")
    args = ap.parse_args()
    if args.one:
        print(json.dumps(measure(args, args.one)), flush=True)
        return
    result = {"samples": args.samples, "sites_per_sample": args.sites, "reps": args.reps, "warmup": args.warmup, "rule": list(RULE),
              "tiles": {}}
    for tile in args.tile_sites:
        cmd = [sys.executable, __file__, "--one", tile, "--samples", args.samples, "--sites", args.sites, "--reps", args.reps,
               "--warmup", args.warmup]
        try:
            r = subprocess.run(list(map(str, cmd)), capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"tile {tile}: no result within {args.step_timeout} s; nothing further is started")
        if r.returncode != 0:
            sys.exit(f"tile {tile}: exit {r.returncode}; nothing further is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        result["tiles"][str(tile)] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(result["tiles"][str(tile)]), file=sys.stderr, flush=True)
    slower = [t for t in args.tile_sites if (result["tiles"][str(t)]["routed_over_fused"] or 2.0) <= 1.0]
    result["crossover_tile_sites"] = min(slower) if slower else None
    level = [t for t in args.tile_sites if result["tiles"][str(t)]["census_over_fused"] <= 1.0]
    result["census_crossover_tile_sites"] = min(level) if level else None
    print(json.dumps(result), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
