#!/usr/bin/env python3
"""What simulating methylomes down a pedigree costs on the device (abn_sim_codes_dev), and what the fit recovers from them.

  1. Kernel time.  Per shape — L in {1 M, 32 M} sites x V in {8, 100} nodes, every node emitted — the HIP-event ms of the
     simulation kernel: 2 warm-up calls, then 9, median and quartiles.  Twice, each in a process of its own: the product
     library (the low words of a draw made only for a quad in which a high word ties) and the measurement build
     (build/libabn_knobs.so with ABN_SIM_BOTH=1: both Philox calls for every quad).  Next to them, in the first process: the
     time hipMemsetAsync takes to write the same bytes (the device's own fill: what writing the matrix costs at the rate
     this device reaches) and the packed pairwise scan's kernel time on the simulated matrix.  The recovery rows' scan_ms is the
     divergence scan and the transition table's pass together.
  2. Recovery.  On the bundled pedigree's shape (tests/golden/data: 9 nodes, 4 sampled) and on an 8-node tree with every
     node sampled, at three (alpha, beta) and L in {1e5, 1e6, 1e7}: simulate.pedigree, then Context.ab_neutral_run
     (p0uu = eqp, weight 1, --starts fits); the recovered alpha and beta next to the truth, and those of a second fit that
     is told the founder's true share of UU sites (0.7) in the place of the measured p0uu.  Nothing is asserted.

Writes one JSON document (--out) and prints its rows.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
SHAPES = [(1 << 20, 8), (1 << 20, 100), (1 << 25, 8), (1 << 25, 100)]
TREE8 = ([-1, 0, 0, 1, 1, 2, 2, 3], [2, 3, 3, 5, 8, 4, 9, 5], [1] * 8)
BUNDLED = ([-1, 0, 0, 1, 2, 3, 4, 5, 6], [0, 1, 1, 1, 1, 3, 3, 4, 4], [1, 1, 0, 0, 0, 0, 0, 1, 1])
RATES = [(2e-3, 5e-3), (5e-4, 1e-3), (1e-4, 1e-4)]


def stats(xs):
    xs = np.asarray(xs, dtype=np.float64)
    q1, med, q3 = np.percentile(xs, [25, 50, 75])
    return {"median": float(med), "q1": float(q1), "q3": float(q3), "min": float(xs.min()), "max": float(xs.max()), "n": int(xs.size)}


def tree(V):
    """V nodes, node v the child of (v - 1) // 2, two generations per level"""
    parent = [-1] + [(v - 1) // 2 for v in range(1, V)]
    generation = [0] * V
    for v in range(1, V):
        generation[v] = generation[parent[v]] + 2
    return (parent, generation, [1] * V) if V != 8 else TREE8


class Hip:
    def __init__(self):
        h = C.CDLL("libamdhip64.so")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipFree.argtypes = [C.c_void_p]
        h.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        h.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        h.hipEventSynchronize.argtypes = [C.c_void_p]
        h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.h = h
        self.e = [C.c_void_p(), C.c_void_p()]
        for e in self.e:
            assert h.hipEventCreate(C.byref(e)) == 0

    def malloc(self, size):
        p = C.c_void_p()
        assert self.h.hipMalloc(C.byref(p), size) == 0
        return p

    def fill_ms(self, ptr, size):
        ms = C.c_float()
        assert self.h.hipEventRecord(self.e[0], None) == 0
        assert self.h.hipMemsetAsync(ptr, 0xFF, size, None) == 0
        assert self.h.hipEventRecord(self.e[1], None) == 0 and self.h.hipEventSynchronize(self.e[1]) == 0
        assert self.h.hipEventElapsedTime(C.byref(ms), *self.e) == 0
        return ms.value


def kernel_child(variant, repeats):
    """one variant's kernel times as a JSON line on stdout (the library is chosen by the parent through the environment)"""
    import alphabeta_rs_amd as abn
    from alphabeta_rs_amd import simulate as S

    ctx, hip = abn.Context(0), Hip()
    rows = []
    for L, V in SHAPES:
        parent, generation, emit = tree(V)
        thr = S.thresholds(parent, generation, 2e-3, 5e-3, 0.7, 0.3)
        stride = abn.packed_row_stride(L)
        buf = hip.malloc(V * stride)
        call = lambda: S.codes_dev(ctx, 20260101, parent, thr, emit, L, buf.value, stride)
        for _ in range(2):
            call()
        row = {"variant": variant, "sites": L, "nodes": V, "bytes": V * stride, "sim_ms": stats([call() for _ in range(repeats)])}
        if variant == "lazy":
            npairs = V * (V - 1) // 2
            dv = hip.malloc(8 * npairs)
            scan = lambda: ctx.pairwise_divergence_packed_dev(buf.value, V, L, stride, 0, 0, dv.value)
            scan()
            row["scan_ms"] = stats([scan() for _ in range(5)])
            hip.h.hipFree(dv)
            scratch = hip.malloc(V * stride)      # another buffer: the simulated matrix stays for nothing, the fill is the fill
            hip.fill_ms(scratch, V * stride)
            row["fill_ms"] = stats([hip.fill_ms(scratch, V * stride) for _ in range(repeats)])
            hip.h.hipFree(scratch)
        hip.h.hipFree(buf)
        rows.append(row)
    ctx.close()
    print("RESULT " + json.dumps(rows))


def recovery(starts):
    import alphabeta_rs_amd as abn
    from alphabeta_rs_amd import simulate as S

    ctx = abn.Context(0)
    rows = []
    for name, (parent, generation, emit) in (("bundled", BUNDLED), ("tree8", TREE8)):
        for alpha, beta in RATES:
            for L in (10 ** 5, 10 ** 6, 10 ** 7):
                ped, p0uu, ms = S.pedigree(ctx, 20260101, parent, generation, emit, alpha, beta, 0.7, 0.3, L, with_ms=True)
                row = {"shape": name, "alpha": alpha, "beta": beta, "sites": L, "p0uu": p0uu, "sim_ms": float(ms[0]), "scan_ms": float(ms[1])}
                try:
                    model, _, _, extra = ctx.ab_neutral_run(ped, p0uu, p0uu, 1.0, starts)
                    row.update(alpha_hat=float(model[0]), beta_hat=float(model[1]), weight_hat=float(model[2]), intercept_hat=float(model[3]),
                               lse=float(np.nanmin(extra["lse"])))
                    told, _, _, _ = ctx.ab_neutral_run(ped, 0.7, 0.7, 1.0, starts)     # the founder's own share of UU sites for p0uu
                    row.update(alpha_hat_told=float(told[0]), beta_hat_told=float(told[1]), weight_hat_told=float(told[2]))
                except abn.AbnError as e:
                    row["error"] = str(e)
                rows.append(row)
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "simulate_ab.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--starts", type=int, default=200)
    ap.add_argument("--child", choices=("lazy", "both"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return kernel_child(a.child, a.repeats)
    from alphabeta_rs_amd import build as B

    kernel = []
    for variant in ("lazy", "both"):
        env = dict(os.environ)
        if variant == "both":
            if not B.KNOBS_LIB.exists():
                sys.exit(f"{B.KNOBS_LIB} is missing: build it first (alphabeta_rs_amd.build.build_knobs())")
            env.update(ABNEUTRAL_HIP_LIB=str(B.KNOBS_LIB), ABN_SIM_BOTH="1")
        r = subprocess.run([sys.executable, __file__, "--child", variant, "--repeats", str(a.repeats)], env=env, capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(f"the {variant} run ended with status {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
        kernel += json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    for row in kernel:
        extra = "".join(f"  {k} {row[k]['median']:.3f}" for k in ("scan_ms", "fill_ms") if k in row)
        print(f"{row['variant']:5s} L {row['sites']:>9d} V {row['nodes']:>3d}  sim {row['sim_ms']['median']:.3f} ms "
              f"[{row['sim_ms']['q1']:.3f}, {row['sim_ms']['q3']:.3f}]{extra}")
    rec = recovery(a.starts)
    for row in rec:
        print(json.dumps(row))
    Path(a.out).parent.mkdir(exist_ok=True)
    Path(a.out).write_text(json.dumps({"kernel": kernel, "recovery": rec}, indent=1) + "\n")


if __name__ == "__main__":
    main()
