#!/usr/bin/env python3
"""A/B of the pairwise scan on 2-bit packed codes against the byte scan of the same sites, in one process, alternating.

Per shape the same seeded random codes are built in both formats on the device; the kernels' HIP-event time of the
device-resident entries (abn_pairwise_divergence_dev / abn_pairwise_divergence_packed_dev: kernel_ms) is taken
--warmup + --reps times, byte and packed run alternating so that both see the same box.  Reported per shape: both
kernel times (median, spread), the code bytes each format holds (what one pass over the codes reads: n x L, n x
row_stride), those bytes over the kernel time as a fraction of 8 TB/s, and the ratio packed / byte.  The condition: packed
is not slower than byte beyond the byte scan's own run-to-run spread (max - min over its median) in this run.

Shapes: the four of DESIGN.md §4's table (15 x 4 M, 15 x 32 M, 50 x 32 M, 50 x 2 M) and 300 x 4 M, where the matrix
pipe and not HBM is expected to bound the scan.  --scale shrinks every length (rehearsal).  For 50 x 32 M the
host-buffer entries are timed end to end as well (host clock; the upload included; --host-reps each, alternating).

Before anything is timed the two formats' results are compared bit for bit, and the device-side packing against
abn_pack_codes on the first rows.  Without a device the script stops after building a small shape in both formats on
the host and checking the oracle on it (no CPU fallback exists).  Prints one JSON line per shape; --out writes them too.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = [(15, 4_000_000), (15, 32_000_000), (50, 32_000_000), (50, 2_000_000), (300, 4_000_000)]
HBM_BPS = 8e12


def stats(xs):
    xs = np.sort(np.asarray(xs, dtype=np.float64))
    med = float(np.median(xs))
    q1, q3 = np.percentile(xs, [25, 75])
    return {"median": med, "min": float(xs[0]), "max": float(xs[-1]), "iqr_over_median": float((q3 - q1) / med),
            "range_over_median": float((xs[-1] - xs[0]) / med), "n": int(xs.size)}


def device_codes(torch, n, L, seed):
    """(n, L) u8 codes on the device: status 0..2, | 0x80 for 8 % of the sites"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    codes = torch.randint(0, 3, (n, L), dtype=torch.uint8, device="cuda", generator=g)
    for i in range(n):      # row by row: the f32 draws of a whole matrix would be four times its size
        codes[i] |= (torch.rand(L, device="cuda", generator=g) < 0.08).to(torch.uint8) << 7
    return codes


def device_pack(torch, codes, stride):
    """the layout of include/abneutral.h with torch ops: site 16 g + 4 j + e -> byte 4 g + e, bits 2j..2j+1"""
    n, L = codes.shape
    packed = torch.empty((n, stride), dtype=torch.uint8, device=codes.device)
    for i in range(n):
        f = torch.full((stride * 4,), 3, dtype=torch.uint8, device=codes.device)
        f[:L] = torch.where(codes[i] >= 0x80, torch.full_like(codes[i], 3), codes[i] & 3)
        f = f.view(stride // 4, 4, 4)                      # [dword g][j][e]
        packed[i] = (f[:, 0] | (f[:, 1] << 2) | (f[:, 2] << 4) | (f[:, 3] << 6)).reshape(stride)
    return packed


def rehearse(A):
    import oracle as O

    O.build()
    rng = np.random.default_rng(1)
    codes = rng.integers(0, 3, size=(7, 3001), dtype=np.uint8)
    codes |= (rng.random(codes.shape) < 0.08).astype(np.uint8) << 7
    packed = A.pack_codes(codes)
    assert np.array_equal(A.unpack_codes(packed, 3001), np.where(codes & 0x80, 0x80, codes))
    wd, wb, _ = O.pairwise_divergence(codes & 3, np.where(codes & 0x80, 0.5, 1.0), 0.99)
    assert wb.max() > 0 and np.all(wd <= 2 * wb)
    return {"device": None, "rehearsal": "host pack / unpack and oracle ok", "packed_bytes": int(packed.nbytes)}


def run_shape(n, L, args, A, torch, ctx):
    stride = A.packed_row_stride(L)
    npairs = n * (n - 1) // 2
    codes = device_codes(torch, n, L, 20261 + n)
    packed = device_pack(torch, codes, stride)
    head = min(n, 2)   # the device-side packing is the library's: the first rows through abn_pack_codes
    assert np.array_equal(packed[:head].cpu().numpy(), A.pack_codes(codes[:head].cpu().numpy()))
    out = {k: [torch.zeros(npairs, dtype=torch.int64, device="cuda"), torch.zeros(npairs, dtype=torch.int64, device="cuda"),
               torch.zeros(npairs, dtype=torch.float64, device="cuda")] for k in ("byte", "packed")}

    def byte():
        return ctx.pairwise_divergence_dev(codes.data_ptr(), n, L, *(o.data_ptr() for o in out["byte"]))

    def pk():
        return ctx.pairwise_divergence_packed_dev(packed.data_ptr(), n, L, stride, *(o.data_ptr() for o in out["packed"]))

    torch.cuda.synchronize()   # the library's stream is not torch's: the inputs are complete before a scan reads them
    byte(), pk()
    torch.cuda.synchronize()
    assert torch.equal(out["byte"][0], out["packed"][0]) and torch.equal(out["byte"][1], out["packed"][1])
    assert torch.equal(out["byte"][2].view(torch.int64), out["packed"][2].view(torch.int64))   # bit for bit, NaN included
    assert int(out["byte"][1].max()) > 0

    t = {"byte": [], "packed": []}
    for rep in range(args.warmup + args.reps):
        row = {"byte": byte(), "packed": pk()}
        if rep >= args.warmup:
            for k, v in row.items():
                t[k].append(v)
    res = {k: stats(v) for k, v in t.items()}
    nbytes = {"byte": n * L, "packed": n * stride}
    info = {"samples": n, "sites": L, "row_stride_bytes": stride, "code_bytes": nbytes,
            "kernel_ms": res,
            "fraction_of_8TBps_over_code_bytes": {k: nbytes[k] / (res[k]["median"] * 1e-3) / HBM_BPS for k in t},
            "ratio_packed_over_byte": res["packed"]["median"] / res["byte"]["median"],
            "packed_not_slower": bool(res["packed"]["median"] <= res["byte"]["median"] * (1.0 + res["byte"]["range_over_median"]))}
    if (n, L) == (50, int(32_000_000 * args.scale)) and args.host_reps > 0:
        h_codes, h_packed = codes.cpu().numpy(), packed.cpu().numpy()
        th = {"byte": [], "packed": []}
        for rep in range(1 + args.host_reps):
            row = {}
            for k, fn in (("byte", lambda: ctx.pairwise_divergence(h_codes)),
                          ("packed", lambda: ctx.pairwise_divergence_packed(h_packed, L))):
                t0 = time.perf_counter()
                r = fn()
                row[k] = (time.perf_counter() - t0) * 1e3
                if rep == 0:
                    assert np.array_equal(r[1].view(np.int64), out["byte"][1].cpu().numpy())
            if rep >= 1:
                for k, v in row.items():
                    th[k].append(v)
        hres = {k: stats(v) for k, v in th.items()}
        info["host_entry_ms"] = hres
        info["host_ratio_packed_over_byte"] = hres["packed"]["median"] / hres["byte"]["median"]
    return info


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every length (0.01: a rehearsal)")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    if args.reps < 1 or args.warmup < 0 or args.host_reps < 0 or not 0 < args.scale <= 1:
        ap.error("--reps >= 1, --warmup >= 0, --host-reps >= 0, 0 < --scale <= 1")
    import torch  # before the product library: one HIP runtime in the process (as bench.py)

    import alphabeta_rs_amd as A

    A.load_library(build_if_missing=True)
    lines = []
    if A.device_count() <= 0:
        print("no HIP device: host packing and oracle only", file=sys.stderr)
        lines.append(rehearse(A))
        print(json.dumps(lines[-1]), flush=True)
    else:
        with A.Context(0) as ctx:
            for n, L in SHAPES:
                info = run_shape(n, int(L * args.scale), args, A, torch, ctx)
                info.update({"reps": args.reps, "warmup": args.warmup, "scale": args.scale})
                lines.append(info)
                print(json.dumps(info), flush=True)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
