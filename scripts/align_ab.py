#!/usr/bin/env python3
"""The price of aligning methylomes (`--align position`, `--align union`), in one process, alternating, from the resident
parse results of every methylome to the finished window handle:

  (a) abn_windows_create_parsed: merge, gene choice, placement — what `--sites device` runs;
  (b) abn_windows_create_aligned: merge, the common-site step of csrc/abn_sites_common.hpp (runs and ends, match, scan and
      rank, gather), then gene choice and placement on the aligned arrays — what `--sites device --align position` runs;
  (c) abn_windows_create_union: merge, the union step of csrc/abn_sites_union.hpp (runs and ends, owner, scan, base, rank,
      dest, invert, gather), then gene choice and placement on n x n_union sites — what `--align union` runs.

All are timed with a host clock around the call (all end in device synchronisations); the parse, identical on all
sides, is outside the span.  The HIP-event times of (b)'s common-site kernels (abn_windows_common) are reported beside
them, and the bytes of the step's temporaries (the formula of sites_common_match and of the RunTables it fills
(csrc/abn_sites_common.hip): the keep flags, the two tables of runs,
match and src of 4 bytes per sample and site of the shortest sample, the workgroup counts; for (c), abn_windows_union and the formula of sites_union_rank / sites_union_gather: owner, P, r and
dest of 4 bytes per site, the tables, the workgroup counts, inv of 4 bytes per sample and union site, own_at).  Shapes, those of
scripts/resident_ab.py with one text for all samples, so that the samples share every site and (b) - (a) is the price of
the step: `lines` = --samples-lines (15) all-context methylomes of --lines (1 000 000) lines, about one in seven CG;
`lines_deferring` = the same with the posterior of every 14th CG line spelled with 23 digits, which the device defers and
the host accepts; `cg` = --samples-cg (8) methylomes of --sites (2 000 000) CG rows on five chromosomes, rows that repeat a
position removed; `cg_thinned` = the same with 1 % of the rows removed at random per sample; `lines_lacking7` and `cg_lacking7` = `lines` and
`cg` with 7 % of the lines removed at random per sample, where the common set shrinks with every sample and the union does
not.  Before anything is timed
the three handles of a shape are compared where the samples share every site: counts, sums bit for bit, layout and packed
bytes.

Prints one JSON line and writes it to --out (default profiles/align_ab.json).
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

import genes_ab  # noqa: E402  (its annotation and CG-row methylome)
import parse_ab  # noqa: E402  (its all-context methylome)
from resident_ab import deferring  # noqa: E402

FIELDS = (("line", np.int64), ("chromosome", np.int32), ("start", np.uint32), ("end", np.uint32), ("strand", np.uint8),
          ("posteriormax", np.float64), ("status", np.uint8), ("meth_lvl", np.float64))


def strictly_ascending(text):
    """the rows of a CG-row methylome without those that repeat the position of the row before them (two rows of one
    position need not come with their strands ascending)"""
    lines = text.split(b"\n")
    out, last = [lines[0]], None
    for l in lines[1:-1]:
        key = l.split(b"\t", 2)[:2]
        if key != last:
            out.append(l)
        last = key
    return b"\n".join(out) + b"\n"


def thinned(text, fraction, seed):
    lines = text.split(b"\n")
    keep = np.random.default_rng(seed).random(len(lines) - 2) >= fraction
    return b"\n".join([lines[0]] + [l for l, k in zip(lines[1:-1], keep) if k]) + b"\n"


def gene_lists(annotation):
    """the annotation as Genes(ctx, lists) takes it: per chromosome the sense, antisense and combined lists, stably sorted
    by start (src/extract.rs:61-66)"""
    genes = {}
    for l in annotation.decode().splitlines():
        f = l.split("\t")
        genes.setdefault(int(f[0]), []).append((int(f[1]), int(f[2]), "+-*".index(f[5]) if f[5] in "+-" else 2))
    lists = []
    for chrom in sorted(genes):
        for kind in range(3):
            lst = sorted((g for g in genes[chrom] if kind == 2 or g[2] == kind), key=lambda g: g[0])
            if lst:
                lists.append((chrom, kind, [g[0] for g in lst], [g[1] for g in lst], [g[2] for g in lst]))
    return lists


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples-lines", type=int, default=15)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--samples-cg", type=int, default=8)
    ap.add_argument("--sites", type=int, default=2_000_000)
    ap.add_argument("--genes", type=int, default=30_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "align_ab.json")
    args = ap.parse_args()
    if args.reps < 10 or args.warmup < 1:
        ap.error("--reps >= 10, --warmup >= 1")
    import alphabeta_rs_amd as A
    from alphabeta_rs_amd import build as B

    A.load_library(build_if_missing=True)
    B.build_host()
    if A.device_count() <= 0:
        sys.exit("no HIP device: both sides build their handle on the device, nothing to time")
    L = C.CDLL(str(B.PEDIGREE_LIB))
    ll = C.c_longlong
    p = lambda t: C.POINTER(t)
    site_ptrs = [p(ll), p(C.c_int), p(C.c_uint), p(C.c_uint), p(C.c_ubyte), p(C.c_double), p(C.c_ubyte), p(C.c_double)]
    L.abh_parse_sites.argtypes = [C.c_char_p, ll, ll, ll, *site_ptrs, p(ll)]
    L.abh_parse_sites.restype = ll

    def decide(text, deferred):
        """the host's parser on every deferred line -> the arrays Sites.insert takes"""
        cols = [[] for _ in FIELDS]
        one = [np.zeros(2, dtype=t) for _, t in FIELDS]
        nw = ll()
        for line, off, n in zip(*(deferred[k].tolist() for k in ("line", "offset", "length"))):
            piece = text[off:off + n]
            got = L.abh_parse_sites(piece, len(piece), 0, 2, *(a.ctypes.data_as(t) for a, t in zip(one, site_ptrs)), C.byref(nw))
            if got == 1:
                cols[0].append(line)
                for c, a in zip(cols[1:], one[1:]):
                    c.append(a[0])
        return [np.array(c, dtype=t) for c, (_, t) in zip(cols, FIELDS)]

    stats = genes_ab.stats
    result = {"reps": args.reps, "warmup": args.warmup, "cutoff": 2048, "step": 5, "size": 5, "absolute": False, "shapes": {}}
    kw = dict(posterior_max_filter=0.99, cutoff=2048, step=5, size=5, absolute=False, counts=(20, 20, 20))

    with A.Context(0) as ctx:
        def run(name, annotation, texts, shared):
            genes = A.Genes(ctx, gene_lists(annotation))
            sites, parsed = [], {}
            for t in texts:                                   # one text object for several samples is parsed once per sample
                r = ctx.parse_sites_resident(t)
                if id(t) not in parsed:
                    parsed[id(t)] = decide(t, r.deferred())
                r.insert(*parsed[id(t)])
                sites.append(r)
            counts = [s.info()["n_sites"] for s in sites]
            info = {"samples": len(texts), "text_bytes": int(sum(map(len, texts))), "sites_min": min(counts), "sites_max": max(counts),
                    "inserted_sample0": int(len(parsed[id(texts[0])][0]))}
            a = A.Windows.from_parsed(ctx, genes, sites, **kw)
            b = A.Windows.from_parsed(ctx, genes, sites, align=True, **kw)
            before, n_common, _ = b.common()
            info["n_common"] = int(n_common)
            n, S, shortest = len(texts), int(before.sum()), int(before.min())
            blocks = (shortest + 255) // 256
            info["temporary_bytes"] = S + 8 * (n + 1) + 2 * 8 * 258 * n + 8 * 4 + 2 * 4 * n * shortest + 4 * (blocks + 1)
            info["merged_array_bytes"] = 22 * S                   # what (b) holds beside (a)'s arrays: the unaligned copies
            u = A.Windows.from_parsed(ctx, genes, sites, align="union", **kw)
            n_union = int(u.union()[1])
            info["n_union"] = n_union
            info["union_temporary_bytes"] = (4 * 4 * S + 4 + 8 * (n + 1) + 2 * 8 * 258 * n + 8 * 4 + 4 * ((S + 255) // 256 + 1) +
                                             3 * 4 * 258 + 4 * n * n_union + 4 * n_union)
            info["union_array_bytes"] = 22 * n * n_union          # the arrays the gene choice and the placement read in (c)
            if shared:
                assert n_common == n_union == min(counts) == max(counts)
                for h in (b, u):
                    for x, y in zip(a.stats() + a.layout() + (a.packed(),), h.stats() + h.layout() + (h.packed(),)):
                        assert x.tobytes() == y.tobytes(), name
                info["equal"] = True
            else:
                assert 0 < n_common < min(counts) and not b.layout()[2].any()
                assert n_union > max(counts) and not u.layout()[2].any()
                info["ragged_windows_unaligned"] = int(a.layout()[2].sum())
            a.close()
            b.close()
            u.close()
            plain, aligned, kernels, union, union_kernels = [], [], [], [], []
            for rep in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                h = A.Windows.from_parsed(ctx, genes, sites, **kw)
                t1 = time.perf_counter()
                h.close()
                t2 = time.perf_counter()
                h = A.Windows.from_parsed(ctx, genes, sites, align=True, **kw)
                t3 = time.perf_counter()
                k = h.common()[2]
                h.close()
                t4 = time.perf_counter()
                h = A.Windows.from_parsed(ctx, genes, sites, align="union", **kw)
                t5 = time.perf_counter()
                ku = h.union()[2]
                h.close()
                if rep >= args.warmup:
                    plain.append(1e3 * (t1 - t0))
                    aligned.append(1e3 * (t3 - t2))
                    union.append(1e3 * (t5 - t4))
                    kernels.append(k)
                    union_kernels.append(ku)
            info["parsed_ms"], info["aligned_ms"] = stats(plain), stats(aligned)
            info["price_ms_median"] = info["aligned_ms"]["median"] - info["parsed_ms"]["median"]
            for i, kname in enumerate(("runs_ends", "match", "scan_rank", "gather")):
                info[f"kernel_ms_{kname}"] = stats([k[i] for k in kernels])
            info["union_ms"] = stats(union)
            info["union_price_ms_median"] = info["union_ms"]["median"] - info["parsed_ms"]["median"]
            for i, kname in enumerate(("runs_ends", "owner", "scan", "base", "rank", "dest", "invert", "gather")):
                info[f"union_kernel_ms_{kname}"] = stats([k[i] for k in union_kernels])
            for s in sites:
                s.close()
            genes.close()
            result["shapes"][name] = info
            print(json.dumps({name: info}), file=sys.stderr, flush=True)

        annotation = (ROOT / "tests" / "golden" / "annotation.txt").read_bytes()
        genes = [(int(f[0]), int(f[1]), int(f[2])) for f in (l.split(b"\t") for l in annotation.splitlines()) if f[0] == b"1"]
        text = parse_ab.methylome(args.lines, 100, genes)
        run("lines", annotation, [text] * args.samples_lines, True)
        run("lines_lacking7", annotation, [thinned(text, 0.07, 300 + s) for s in range(args.samples_lines)], False)
        text = deferring(text, 14)
        run("lines_deferring", annotation, [text] * args.samples_lines, True)
        span = 24_000_000
        synthetic = genes_ab.annotation(args.genes, span, 7)
        text = strictly_ascending(genes_ab.methylome(args.sites, span, 100))
        run("cg", synthetic, [text] * args.samples_cg, True)
        run("cg_thinned", synthetic, [thinned(text, 0.01, 200 + s) for s in range(args.samples_cg)], False)
        run("cg_lacking7", synthetic, [thinned(text, 0.07, 400 + s) for s in range(args.samples_cg)], False)
    print(json.dumps(result), flush=True)
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
