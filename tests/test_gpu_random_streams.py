"""The Philox streams at full-width counters: a 64-bit seed whose high word is not zero (the key's second word), window
ids and a bootstrap offset with their top bits set.  The host generators and every device code path that derives the key
itself — abn_gen_idx_kernel and the jitter of abn_fit_kernel, abn_fit_refill_kernel, abn_fit_spec_kernel and
abn_sweep_kernel — against the oracle at the same seed, ids and offsets, bit for bit.  A narrowing of the seed, the window
id or the bootstrap offset anywhere between the ABI, the binding, the launch arguments and a kernel's key set-up changes
the stream and fails here.

No counter wraps past 2^32: wrap-around is not a contract.  Where a call needs more than the 256 bootstraps BOOT0 leaves
below 2^32 (the grid-stride call of abn_gen_idx_kernel, the persistent launch), its offset is 2^32 minus its count.
"""
import numpy as np
import pytest

from alphabeta_rs_amd import synthetic

import _kernel_matrix as KM
from _parity import assert_fits_equal, check_selection_and_boot, run_plan, sample_chains, synthetic_pedigree

SEED64 = 0x9E3779B97F4A7C15
SEED_LOW = SEED64 & 0xFFFFFFFF          # the same low word, high word 0: what a truncated seed would draw from
IDS = (0xFFFFFFFF, 0x80000000, 7)
BOOT0 = 0xFFFFFF00
WINDOW = 0x80000001
P0 = synthetic.TRUE_P0UU
SCALE = (1.0, 0.85, 1.2)                # the windows' observations: the pedigree's, scaled


def _offset_for(nb):
    """BOOT0, or the largest offset at which bootstrap nb - 1 still has a counter below 2^32"""
    return min(BOOT0, (1 << 32) - nb)


# ------------------------------------------------------------------------------------------------ host generators (no GPU)
def test_host_start_simplices_at_full_width(abn, oracle):
    n, max_div = 6, 0.0123
    got = abn.gen_start_simplices(SEED64, IDS[0], n, max_div)
    want = np.stack([oracle.start_simplex(SEED64, IDS[0], s, max_div) for s in range(n)])
    assert got.tobytes() == want.tobytes()
    low = np.stack([oracle.start_simplex(SEED_LOW, IDS[0], s, max_div) for s in range(n)])
    assert abn.gen_start_simplices(SEED_LOW, IDS[0], n, max_div).tobytes() == low.tobytes() != want.tobytes()
    for other in (IDS[0] & 0x7FFFFFFF, IDS[0] & 0xFFFF):       # a window id cut to 31 or 16 bits is another stream
        assert abn.gen_start_simplices(SEED64, other, n, max_div).tobytes() != want.tobytes()


def test_host_boot_simplices_at_full_width(abn, oracle):
    nb, params = 7, synthetic.TRUE_PARAMS
    got = abn.gen_boot_simplices(SEED64, IDS[0], BOOT0, nb, params)
    want = np.stack([oracle.boot_simplex(SEED64, IDS[0], BOOT0 + b, params) for b in range(nb)])
    assert got.tobytes() == want.tobytes()
    low = np.stack([oracle.boot_simplex(SEED_LOW, IDS[0], BOOT0 + b, params) for b in range(nb)])
    assert abn.gen_boot_simplices(SEED_LOW, IDS[0], BOOT0, nb, params).tobytes() == low.tobytes() != want.tobytes()
    for other in (BOOT0 & 0x7FFFFFFF, BOOT0 & 0xFFFF):
        assert abn.gen_boot_simplices(SEED64, IDS[0], other, nb, params).tobytes() != want.tobytes()


# ------------------------------------------------------------------------------------------------ stand-alone indices
def _indices_against_oracle(gpu_ctx, oracle, n, nb):
    """both seeds against the oracle, every row; returns whether the oracle's two tables differ"""
    b0 = _offset_for(nb)
    assert b0 + nb <= 1 << 32
    tables = []
    for seed in (SEED64, SEED_LOW):
        got = gpu_ctx.gen_boot_indices(seed, WINDOW, b0, nb, n)
        want = np.stack([oracle.boot_indices(seed, WINDOW, b0 + b, n) for b in range(nb)])
        assert got.dtype == np.uint32 and got.shape == (nb, n)
        bad = np.flatnonzero(np.any(got != want, axis=1))
        assert bad.size == 0, (n, hex(seed), bad[:8])
        assert want.max() < n
        tables.append(got)
    return not np.array_equal(tables[0], tables[1])


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 8, 1024))
def test_boot_indices_at_full_width(gpu_ctx, oracle, n):
    """N a multiple of 4 (4, 8, 1024): every element of the last quad is inside the row; N = 1, 2, 3, 5: it is cut.  With
    one row every index is 0 whatever the stream: there the two seeds cannot differ, everywhere else they must."""
    differ = _indices_against_oracle(gpu_ctx, oracle, n, 3)
    assert differ == (n > 1), n


@pytest.mark.gpu
def test_boot_indices_past_one_grid(gpu_ctx, oracle):
    """abn_gen_idx_kernel's grid is capped at 32 blocks of 256 threads per CU, one quad of a row per thread: more quads than
    that and every thread takes another trip of the grid-stride loop"""
    cus = gpu_ctx.device_info()["compute_units"]
    n = 4001
    quads = (n + 3) // 4
    assert quads == 1001
    nb = (32 * cus * 256 * 105 // 100) // quads + 1
    assert nb * 1001 > 32 * cus * 256 * 1.05
    assert _indices_against_oracle(gpu_ctx, oracle, n, nb)


# ------------------------------------------------------------------------------------------------ jitter: one plan per path
def _windows(ped, W):
    return np.stack([ped[:, 3] * SCALE[w] for w in range(W)])


def _check_plan(abn, oracle, ped, D, ids, S, ia, ib, boot_offset, out, o, label, rows=None, table=True):
    """starts, selection and bootstrap rows of every window against the oracle at the plan's seed, ids and offset"""
    tree = abn.reduction_tree(ped[:, :3], o)
    assert np.all(out["info_a"]["lanes"] == tree) and np.all(out["info_b"]["lanes"] == tree), label
    for w, wid in enumerate(ids):
        pw = np.concatenate([ped[:, :3], D[w][:, None]], axis=1)
        s0 = abn.gen_start_simplices(SEED64, wid, S, D[w].max())
        fits = oracle.fit_batch(pw, P0, P0, 1.0, s0, ia, lanes=tree, table=table, threads=4)
        assert_fits_equal(None, out["info_a"][w], fits, (label, w))
        check_selection_and_boot(oracle, pw, P0, out, fits["best"], SEED64, ib, tree, (label, w), rows=rows, window=w,
                                 ids=ids, boot_offset=boot_offset)


STREAM16 = (KM.FIT, 16, 0, False, False, False)    # the 16-lane streamed case whose own stream_mode is 0 (N = 769)
JITTER = {  # path: (MATRIX case, option overrides, kernel kind of both phases)
    "fit_resident": ((KM.FIT, 8, 1, False, False, False), {}, "resident"),
    "fit_streamed_materialised": (STREAM16, {"stream_mode": 0}, "stream"),
    "fit_streamed_gathered": (STREAM16, {"stream_mode": 1}, "stream"),
    "spec": ((KM.SPEC, 64, 1, False, False, False), {}, "speculative"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(JITTER))
def test_jitter_at_full_width(abn, gpu_ctx, oracle, path):
    key, override, kind = JITTER[path]
    c = KM.MATRIX[key]
    opts = dict(c["opts"], **override)
    assert isinstance(c["B"], int) and c["B"] <= (1 << 32) - BOOT0
    if key[0] == KM.FIT and key[2] <= 0:
        assert c["opts"]["stream_mode"] == 0           # a streamed case: both forms of the bootstrap observations apply
    ped = KM.pedigree(c)
    o = abn.default_options(seed=SEED64, **opts)
    D = _windows(ped, len(IDS))
    out, kinds, _ = run_plan(abn, gpu_ctx, ped, P0, c["S"], c["B"], o, boot_offset=BOOT0, ids=IDS, D=D)
    lanes = 64 if key[0] == KM.SPEC else key[1]
    assert kinds == {"starts": (kind, lanes), "boot": (kind, lanes)}, (path, kinds)
    _check_plan(abn, oracle, ped, D, IDS, c["S"], opts["max_iters_start"], opts["max_iters_boot"], BOOT0, out, o, path)


@pytest.mark.gpu
def test_jitter_at_full_width_persistent(abn, gpu_ctx, oracle):
    """abn_fit_refill_kernel: one window (id 2^32 - 1), more bootstraps than a persistent launch's wavefronts hold lane
    groups, so the offset is 2^32 minus their number; sampled rows, the first and the last among them"""
    key = (KM.REFILL, 8, 1, False, False, False)
    c = KM.MATRIX[key]
    dev = gpu_ctx.device_info()
    B = KM.boot_count(c, dev["persistent_wavefronts_small"], dev["compute_units"])
    boot_offset = _offset_for(B)
    assert boot_offset >= 0xFFFF0000 and boot_offset + B == 1 << 32
    ped = KM.pedigree(c)
    o = abn.default_options(seed=SEED64, **c["opts"])
    ids = IDS[:1]
    D = _windows(ped, 1)
    out, kinds, _ = run_plan(abn, gpu_ctx, ped, P0, c["S"], B, o, boot_offset=boot_offset, ids=ids, D=D)
    assert kinds == {"starts": ("resident", 8), "boot": ("persistent", 8)}, kinds
    _check_plan(abn, oracle, ped, D, ids, c["S"], c["opts"]["max_iters_start"], c["opts"]["max_iters_boot"], boot_offset,
                out, o, "refill", rows=sample_chains(B, 8))


@pytest.mark.gpu
def test_jitter_at_full_width_sweep(abn, gpu_ctx, oracle):
    """abn_sweep_kernel: a streamed 64-lane plan (N = 1100) with the sweep switched on"""
    ped = synthetic_pedigree(np.random.default_rng(11), 1100, 12)
    S, B, ia, ib = 3, 5, 50, 30
    o = abn.default_options(seed=SEED64, max_iters_start=ia, max_iters_boot=ib)
    assert abn.reduction_tree(ped[:, :3], o) == 64 | (3 << 8)
    D = _windows(ped, len(IDS))
    out, kinds, _ = run_plan(abn, gpu_ctx, ped, P0, S, B, o, boot_offset=BOOT0, ids=IDS, D=D, sweep=1)
    assert kinds == {"starts": ("stream_sweep", 64), "boot": ("stream_sweep", 64)}, kinds
    _check_plan(abn, oracle, ped, D, IDS, S, ia, ib, BOOT0, out, o, "sweep")
