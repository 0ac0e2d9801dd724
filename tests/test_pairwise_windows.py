"""abn_pairwise_divergence_windows / _windows_dev: the pairwise divergence (DMatrix::from, src/pedigree.rs:210-261) of many
column ranges of one code matrix in one batched call (the window loop of src/cli/metaprofile.rs:50-72), against the oracle
on every slice and against the per-window entry, bit for bit; and Pedigree::build_many on top of it against the host loop
of Pedigree::build."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
CHUNK_SITES = 8192      # kPmxWinChunkSites (csrc/abn_pairwise_windows.hpp): longer windows are cut into chunks
MAX_JOBS = 8192         # kPmxMaxJobs (csrc/abn_pairwise.hip): jobs per launch


def _codes(status, pmax, flt):
    return (status | np.where(pmax < flt, 0x80, 0)).astype(np.uint8)


def _random(seed, n, stride):
    rng = np.random.default_rng(seed)
    status = rng.integers(0, 3, size=(n, stride), dtype=np.uint8)
    pmax = rng.uniform(0.9, 1.0, size=(n, stride))
    pmax[0, : stride // 2] = 0.5                 # a sample with a long filtered stretch
    if n > 2:
        pmax[2] = 0.1                            # a sample with no valid site at all -> 0/0 = NaN like the reference
    return status, pmax, _codes(status, pmax, 0.99)


def _check_against_oracle(oracle, got, status, pmax, begin, end):
    diff, both, dval = got
    for w, (b, e) in enumerate(zip(begin, end)):
        wd, wb, wv = oracle.pairwise_divergence(status[:, b:e], pmax[:, b:e], 0.99)
        assert np.array_equal(diff[w], wd) and np.array_equal(both[w], wb), (w, b, e)
        assert np.array_equal(dval[w], wv, equal_nan=True), (w, b, e)


STRIDE = 6001
EDGE_LENGTHS = [0, 1, 3, 4, 63, 64, 65, 127, 128, 129, 1000, 2049]


def _edge_windows():
    """begins over every residue mod 4 and several mod 64; the lengths above; overlaps (each begin is inside the previous
    window for the long ones), gaps (after the short ones); one at 0, one ending at the row's end, one over the whole row"""
    begin, end = [], []
    pos = 0
    for k, ln in enumerate(EDGE_LENGTHS * 3):
        b = pos + k % 4 + (17 * k) % 64          # k % 4 walks the residues mod 4
        b = min(b, STRIDE - ln)
        begin.append(b)
        end.append(b + ln)
        pos = (b + ln // 2 + 5) % (STRIDE - 2100)
    begin += [0, 0, STRIDE - 129, STRIDE - 1, 0, STRIDE, 2]
    end += [64, 1, STRIDE, STRIDE, STRIDE, STRIDE, STRIDE - 3]
    return np.array(begin, dtype=np.int64), np.array(end, dtype=np.int64)


@pytest.mark.parametrize("n", [2, 15, 17, 64, 65, 130])
def test_windows_edges(abn, gpu_ctx, oracle, n):
    status, pmax, codes = _random(n, n, STRIDE)
    begin, end = _edge_windows()
    assert STRIDE % 4 and {int(b) % 4 for b in begin} == {0, 1, 2, 3} and len({int(b) % 64 for b in begin}) >= 8
    assert len(begin) >= 40 and set(EDGE_LENGTHS) <= {int(x) for x in end - begin}
    assert np.any(begin[1:] < end[:-1]) and np.any(begin[1:] > end[:-1])          # overlaps and gaps
    got = gpu_ctx.pairwise_divergence_windows(codes, begin, end)
    _check_against_oracle(oracle, got, status, pmax, begin, end)
    for w, (b, e) in enumerate(zip(begin, end)):                                  # the old entry on each slice
        od, ob, ov = gpu_ctx.pairwise_divergence(codes[:, b:e])
        assert np.array_equal(got[0][w], od) and np.array_equal(got[1][w], ob)
        assert np.array_equal(got[2][w], ov, equal_nan=True)
        if b == e:
            assert np.all(got[1][w] == 0) and np.all(got[0][w] == 0) and np.all(np.isnan(got[2][w]))


def test_windows_every_state_pair_through_the_edges(abn, gpu_ctx, oracle):
    """Every (state_a, state_b) combination of {U, I, M, filtered U/I/M} in known counts on two samples of different
    16-blocks and groups, the crafted columns straddling a window's begin and another's end: a site counted from outside
    the window, or a transposed tile, shows."""
    n, reps = 150, 37
    states = np.array([0, 1, 2, 0x80, 0x81, 0x82], dtype=np.uint8)
    rng = np.random.default_rng(7)
    codes = states[rng.integers(0, 6, size=(n, 36 * reps))]
    a, b = 3, 141
    cols = []
    for ia, sa in enumerate(states):
        for ib, sb in enumerate(states):
            cols += [(sa, sb)] * ((6 * ia + ib) % 5 + 1)
    cols = np.array(cols, dtype=np.uint8)
    at = 301                                            # the crafted columns are [at, at + len(cols))
    codes[a, at: at + len(cols)] = cols[:, 0]
    codes[b, at: at + len(cols)] = cols[:, 1]
    mid = at + len(cols) // 2 + 1
    begin = np.array([at + 7, 13, at, at - 3, mid, at + 1], dtype=np.int64)
    end = np.array([at + len(cols) + 50, mid, at + len(cols), at + len(cols) - 2, codes.shape[1], at + 2], dtype=np.int64)
    got = gpu_ctx.pairwise_divergence_windows(codes, begin, end)
    status, pmax = codes & 3, np.where(codes & 0x80, 0.5, 1.0)
    _check_against_oracle(oracle, got, status, pmax, begin, end)


def test_windows_a_chunked_window_among_short_ones(abn, gpu_ctx, oracle):
    n, long_len = 9, 1_000_003
    assert long_len > CHUNK_SITES                        # the long window takes the chunked path, the others do not
    rng = np.random.default_rng(11)
    lens = rng.integers(50, 5001, size=11)
    assert lens.max() <= CHUNK_SITES
    stride = 1_020_001
    status, pmax, codes = _random(12, n, stride)
    short_b = rng.integers(0, stride - 5000, size=11)
    begin = np.concatenate([short_b[:6], [9_999], short_b[6:]]).astype(np.int64)
    end = np.concatenate([short_b[:6] + lens[:6], [9_999 + long_len], short_b[6:] + lens[6:]]).astype(np.int64)
    got = gpu_ctx.pairwise_divergence_windows(codes, begin, end)
    _check_against_oracle(oracle, got, status, pmax, begin, end)


def test_windows_job_indexing(abn, gpu_ctx, oracle):
    """n = 70: two diagonal super-pairs and one off-diagonal, 300 windows of 40-900 sites."""
    n, W, stride = 70, 300, 20_003
    status, pmax, codes = _random(70, n, stride)
    rng = np.random.default_rng(3)
    lens = rng.integers(40, 901, size=W)
    begin = rng.integers(0, stride - 900, size=W).astype(np.int64)
    got = gpu_ctx.pairwise_divergence_windows(codes, begin, begin + lens)
    _check_against_oracle(oracle, got, status, pmax, begin, begin + lens)


def test_windows_more_jobs_than_one_launch_holds(abn, gpu_ctx, oracle):
    """n = 65 has two diagonal super-pairs: 4100 windows are 8200 jobs of that family, more than one launch takes."""
    n, W, stride = 65, 4100, 4 * 4100 + 41
    assert 2 * W > MAX_JOBS
    status, pmax, codes = _random(65, n, stride)
    begin = (4 * np.arange(W) + np.arange(W) % 3).astype(np.int64)
    end = begin + 40
    got = gpu_ctx.pairwise_divergence_windows(codes, begin, end)
    _check_against_oracle(oracle, got, status, pmax, begin, end)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_windows_device_resident_entry(abn, gpu_ctx, oracle, shift):
    """Codes and results stay in HBM; the codes start `shift` bytes off an aligned allocation; each output NULL in turn.
    The device buffers come from the HIP runtime the product library already holds, as in
    tests/test_pairwise.py::test_gpu_pairwise_device_resident_entry (a torch imported after it would bring a second copy
    of the runtime into the process); a torch tensor's data_ptr() is passed the same way (scripts/pairwise_windows_ab.py)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    n, stride = 21, 30_000
    status, pmax, codes = _random(shift, n, stride)
    rng = np.random.default_rng(shift)
    W = 12
    begin = rng.integers(0, stride - 20_000, size=W).astype(np.int64)
    lens = rng.integers(0, 20_000, size=W)
    lens[0], begin[1], lens[1] = 0, stride - 9000, 9000       # an empty window; one to the end of the last row
    end = begin + lens
    nout = W * (n * (n - 1) // 2)
    want = gpu_ctx.pairwise_divergence_windows(codes, begin, end)
    _check_against_oracle(oracle, want, status, pmax, begin, end)
    bufs = [C.c_void_p() for _ in range(4)]
    for ptr, size in zip(bufs, (codes.nbytes + 16, 8 * nout, 8 * nout, 8 * nout)):
        assert hip.hipMalloc(C.byref(ptr), size) == 0
    try:
        assert bufs[0].value % 4 == 0
        dcodes = bufs[0].value + shift
        assert hip.hipMemcpy(C.c_void_p(dcodes), codes.ctypes.data, codes.nbytes, 1) == 0
        for skip in (None, 0, 1, 2):                          # all three outputs; then each of them NULL in turn
            for ptr in bufs[1:]:
                assert hip.hipMemset(ptr, 7, 8 * nout) == 0
            ptrs = [0 if k == skip else bufs[1 + k].value for k in range(3)]
            ms = gpu_ctx.pairwise_divergence_windows_dev(dcodes, n, stride, begin, end, *ptrs)
            assert ms > 0
            for k in range(3):
                host = np.zeros(nout, dtype=np.float64 if k == 2 else np.uint64)
                assert hip.hipMemcpy(host.ctypes.data, bufs[1 + k], 8 * nout, 2) == 0
                if k == skip:
                    assert np.all(host.view(np.uint8) == 7)   # untouched
                else:
                    assert np.array_equal(host, want[k].reshape(-1), equal_nan=(k == 2))
    finally:
        for ptr in bufs:
            hip.hipFree(ptr)


def test_windows_arguments(abn, gpu_ctx):
    codes = np.zeros((3, 100), dtype=np.uint8)
    for b, e in (([5], [4]), ([0], [101]), ([-1], [10]), ([0, 50], [10, 49])):
        with pytest.raises(abn.AbnError) as err:
            gpu_ctx.pairwise_divergence_windows(codes, b, e)
        assert err.value.status == 1
    i64p = C.POINTER(C.c_int64)
    one = np.zeros(1, dtype=np.int64)
    rc = gpu_ctx._L.abn_pairwise_divergence_windows(gpu_ctx._h, codes.ctypes.data_as(C.POINTER(C.c_uint8)), 3, 100,
                                                    one.ctypes.data_as(i64p), one.ctypes.data_as(i64p), -1, None, None, None)
    assert rc == 1
    rc = gpu_ctx._L.abn_pairwise_divergence_windows(gpu_ctx._h, None, 3, 100, one.ctypes.data_as(i64p),
                                                    one.ctypes.data_as(i64p), 1, None, None, None)
    assert rc == 1
    d, b, v = gpu_ctx.pairwise_divergence_windows(codes, [], [])                  # no windows
    assert d.shape == (0, 3) and b.shape == (0, 3) and v.shape == (0, 3)
    d, b, v = gpu_ctx.pairwise_divergence_windows(codes[:1], [0, 10], [10, 20])   # one sample: no pairs
    assert d.shape == (2, 0) and v.size == 0


def test_build_many_on_the_gpu(abn, gpu_ctx, tmp_path):
    """Pedigree::build_many with the batched scan against Pedigree::build's host loop per window: windows with their own
    methylomes (different row slices of the bundled ones), a missing nodelist, a three-sample window and one whose samples
    have unequal lengths."""
    from _build_many import build_each, build_many, hostlib, write_windows

    L = hostlib()
    lists = write_windows(tmp_path, GOLDEN)
    many = build_many(L, lists, gpu=True)
    each = build_each(L, lists)
    assert [m[0] for m in many] == [6, 6, -1, 3, 6, 6, 6]
    assert b"could not read nodelist" in many[2][3]
    for m, e in zip(many, each):
        assert m[0] == e[0] and m[3] == e[3]
        if m[0] >= 0:
            assert m[1].tobytes() == e[1].tobytes() and m[2] == e[2]
    assert len({m[1].tobytes() for m in many if m[0] == 6}) == 5      # the windows do differ
