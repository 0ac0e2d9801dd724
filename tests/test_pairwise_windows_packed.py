"""abn_pairwise_divergence_windows_packed / _windows_packed_dev: the pairwise divergence (DMatrix::from,
src/pedigree.rs:210-261) of many column ranges of one 2-bit packed code matrix in one batched call (the window loop of
src/cli/metaprofile.rs:50-72).  Inputs are abn.pack_codes of random byte codes; every result is compared bit for bit
(equal_nan for dvalue) with the oracle on each slice and with pairwise_divergence_windows on the same byte codes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PACKED_CHUNK_SITES = 32768   # kPmxWinPackedChunkSites (csrc/abn_packed_mask.hpp): longer windows are cut into chunks
MAX_JOBS = 8192              # kPmxMaxJobs (csrc/abn_pairwise.hip): jobs per launch
INVALID = 1                  # ABN_ERR_INVALID_ARG


def _codes(status, pmax, flt):
    return (status | np.where(pmax < flt, 0x80, 0)).astype(np.uint8)


def _random(seed, n, sites):
    rng = np.random.default_rng(seed)
    status = rng.integers(0, 3, size=(n, sites), dtype=np.uint8)
    pmax = rng.uniform(0.9, 1.0, size=(n, sites))
    pmax[0, : sites // 2] = 0.5                  # a sample with a long filtered stretch
    if n > 2:
        pmax[2] = 0.1                            # a sample with no valid site at all -> 0/0 = NaN like the reference
    return status, pmax, _codes(status, pmax, 0.99)


def _check_against_oracle(oracle, got, status, pmax, begin, end):
    diff, both, dval = got
    for w, (b, e) in enumerate(zip(begin, end)):
        wd, wb, wv = oracle.pairwise_divergence(status[:, b:e], pmax[:, b:e], 0.99)
        assert np.array_equal(diff[w], wd) and np.array_equal(both[w], wb), (w, b, e)
        assert np.array_equal(dval[w], wv, equal_nan=True), (w, b, e)


def _check_equal(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2], equal_nan=True)


SITES = 6001
EDGE_LENGTHS = [0, 1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 2049]


def _edge_windows():
    """48 windows of the lengths above whose begins walk the residues mod 16 (overlaps: each begin is inside the previous
    window for the long ones; gaps after the short ones), then begins on both sides of multiples of 64 and 256, windows
    inside one dword and inside one super-step, one at 0, one ending at the row's end, the whole row, an empty one at
    the row's end"""
    begin, end = [], []
    pos = 0
    for k, ln in enumerate(EDGE_LENGTHS * 3):
        b = pos // 16 * 16 + k % 16
        b = min(b, SITES - ln)
        begin.append(b)
        end.append(b + ln)
        pos = (b + ln // 2 + 5) % (SITES - 2100)
    extra = [(63, 66), (64, 65), (65, 70), (255, 258), (256, 512), (257, 300), (1023, 1025), (1024, 1280), (1025, 1279),
             (37, 40), (33, 47), (300, 500), (515, 767),                # inside one dword; inside one super-step
             (0, 64), (0, 1), (SITES - 129, SITES), (SITES - 1, SITES), (0, SITES), (SITES, SITES), (2, SITES - 3)]
    begin += [b for b, _ in extra]
    end += [e for _, e in extra]
    return np.array(begin, dtype=np.int64), np.array(end, dtype=np.int64)


def _assert_edge_window_set(begin, end):
    b, e = [int(x) for x in begin], [int(x) for x in end]
    assert len(b) >= 48 and set(EDGE_LENGTHS) <= {y - x for x, y in zip(b, e)}
    assert {x % 16 for x in b} == set(range(16))
    assert {63, 0, 1} <= {x % 64 for x in b} and {255, 0, 1} <= {x % 256 for x in b}
    assert len({x % 256 for x in b}) >= 8
    assert any(x < y and x // 16 == (y - 1) // 16 and x % 16 and y % 16 for x, y in zip(b, e))      # inside one dword
    assert any(x // 16 != (y - 1) // 16 and x // 256 == (y - 1) // 256 and x % 256 and y % 256 for x, y in zip(b, e))
    assert np.any(begin[1:] < end[:-1]) and np.any(begin[1:] > end[:-1])                             # overlaps and gaps
    pairs = set(zip(b, e))
    assert (0, SITES) in pairs and (SITES, SITES) in pairs
    assert any(x == 0 and y < SITES for x, y in pairs) and any(x > 0 and y == SITES for x, y in pairs)


@pytest.mark.parametrize("n", [2, 17, 65, 130])
def test_packed_windows_edges(abn, gpu_ctx, oracle, n):
    status, pmax, codes = _random(n, n, SITES)
    packed = abn.pack_codes(codes)
    assert packed.shape == (n, 1536)
    begin, end = _edge_windows()
    _assert_edge_window_set(begin, end)
    got = gpu_ctx.pairwise_divergence_windows_packed(packed, SITES, begin, end)
    _check_against_oracle(oracle, got, status, pmax, begin, end)
    _check_equal(got, gpu_ctx.pairwise_divergence_windows(codes, begin, end))
    for w in np.flatnonzero(begin == end):
        assert np.all(got[0][w] == 0) and np.all(got[1][w] == 0) and np.all(np.isnan(got[2][w]))


def test_packed_windows_every_state_pair_through_the_edges(abn, gpu_ctx, oracle):
    """All 4 x 4 combinations of U / I / M / filtered in known, different counts on two samples of different 16-blocks and
    groups, the crafted columns straddling one window's begin and another's end: a site counted from outside the window,
    or a transposed tile, shows."""
    n, sites = 150, 1400
    states = np.array([0, 1, 2, 0x80], dtype=np.uint8)
    rng = np.random.default_rng(7)
    codes = states[rng.integers(0, 4, size=(n, sites))]
    a, b = 3, 141
    cols, counts = [], {}
    for ia, sa in enumerate(states):
        for ib, sb in enumerate(states):
            counts[(ia, ib)] = 2 * (4 * ia + ib) + 1                      # 1, 3, ..., 31: all different
            cols += [(sa, sb)] * counts[(ia, ib)]
    assert len(set(counts.values())) == 16
    cols = np.array(cols, dtype=np.uint8)
    cols = cols[rng.permutation(len(cols))]
    at = 301                                                              # the crafted columns are [at, at + len(cols))
    assert at // 256 != (at + len(cols) - 1) // 256                       # ... and straddle a super-step boundary
    codes[a, at: at + len(cols)] = cols[:, 0]
    codes[b, at: at + len(cols)] = cols[:, 1]
    mid = at + len(cols) // 2 + 1
    begin = np.array([at + 7, 13, at, at - 3, mid, at + 1], dtype=np.int64)
    end = np.array([at + len(cols) + 50, mid, at + len(cols), at + len(cols) - 2, sites, at + 2], dtype=np.int64)
    got = gpu_ctx.pairwise_divergence_windows_packed(abn.pack_codes(codes), sites, begin, end)
    status, pmax = codes & 3, np.where(codes & 0x80, 0.5, 1.0)
    _check_against_oracle(oracle, got, status, pmax, begin, end)
    # the window that is exactly the crafted columns, pair (a, b): the counts above, by hand
    p = a * n - a * (a + 1) // 2 + (b - a - 1)
    want_both = sum(c for (ia, ib), c in counts.items() if ia < 3 and ib < 3)
    want_diff = sum(c * abs(ia - ib) for (ia, ib), c in counts.items() if ia < 3 and ib < 3)
    assert got[1][2][p] == want_both and got[0][2][p] == want_diff


def test_packed_windows_outside_does_not_count(abn, gpu_ctx):
    """The same windows on two packed matrices that differ only in fields outside every window."""
    n, sites = 21, 3001
    rng = np.random.default_rng(21)
    states = np.array([0, 1, 2, 0x80], dtype=np.uint8)
    codes = states[rng.integers(0, 4, size=(n, sites))]
    begin = np.array([5, 100, 250, 300, 700, 1029, 1500, 2303, 2990], dtype=np.int64)
    end = np.array([6, 131, 263, 600, 1023, 1030, 2049, 2817, 2999], dtype=np.int64)
    inside = np.zeros(sites, dtype=bool)
    for b, e in zip(begin, end):
        inside[b:e] = True
    assert inside.sum() < sites - 500 and not inside[0] and not inside[-1]
    other = codes.copy()
    other[:, ~inside] = states[(np.searchsorted(states, codes[:, ~inside]) + rng.integers(1, 4, size=(n, (~inside).sum()))) % 4]
    assert np.all(other[:, ~inside] != codes[:, ~inside]) and np.array_equal(other[:, inside], codes[:, inside])
    pa, pb = abn.pack_codes(codes), abn.pack_codes(other)
    assert not np.array_equal(pa, pb)
    ga = gpu_ctx.pairwise_divergence_windows_packed(pa, sites, begin, end)
    _check_equal(gpu_ctx.pairwise_divergence_windows_packed(pb, sites, begin, end), ga)
    _check_equal(ga, gpu_ctx.pairwise_divergence_windows(codes, begin, end))
    assert ga[1].max() > 0


def test_packed_windows_a_chunked_window_among_short_ones(abn, gpu_ctx, oracle):
    n, long_len = 9, 1_000_003
    assert long_len > PACKED_CHUNK_SITES                 # the long window takes the chunked path, the others do not
    rng = np.random.default_rng(11)
    lens = rng.integers(50, 5001, size=11)
    assert lens.max() + 255 <= PACKED_CHUNK_SITES        # (a window's chunks count from the super-step of its begin)
    sites = 1_020_001
    status, pmax, codes = _random(12, n, sites)
    short_b = rng.integers(0, sites - 5000, size=11)
    begin = np.concatenate([short_b[:6], [9_999], short_b[6:]]).astype(np.int64)
    end = np.concatenate([short_b[:6] + lens[:6], [9_999 + long_len], short_b[6:] + lens[6:]]).astype(np.int64)
    got = gpu_ctx.pairwise_divergence_windows_packed(abn.pack_codes(codes), sites, begin, end)
    _check_against_oracle(oracle, got, status, pmax, begin, end)
    _check_equal(got, gpu_ctx.pairwise_divergence_windows(codes, begin, end))


def test_packed_windows_job_indexing(abn, gpu_ctx, oracle):
    """n = 70: two diagonal super-pairs and one off-diagonal, 300 windows of 40-900 sites."""
    n, W, sites = 70, 300, 20_003
    status, pmax, codes = _random(70, n, sites)
    rng = np.random.default_rng(3)
    lens = rng.integers(40, 901, size=W)
    begin = rng.integers(0, sites - 900, size=W).astype(np.int64)
    got = gpu_ctx.pairwise_divergence_windows_packed(abn.pack_codes(codes), sites, begin, begin + lens)
    _check_against_oracle(oracle, got, status, pmax, begin, begin + lens)


def test_packed_windows_more_jobs_than_one_launch_holds(abn, gpu_ctx, oracle):
    """n = 65 has two diagonal super-pairs: 4100 windows are 8200 jobs of that family, more than one launch takes."""
    n, W, sites = 65, 4100, 4 * 4100 + 41
    assert 2 * W > MAX_JOBS
    status, pmax, codes = _random(65, n, sites)
    begin = (4 * np.arange(W) + np.arange(W) % 3).astype(np.int64)
    end = begin + 40
    got = gpu_ctx.pairwise_divergence_windows_packed(abn.pack_codes(codes), sites, begin, end)
    _check_against_oracle(oracle, got, status, pmax, begin, end)


def test_packed_windows_device_resident_entry(abn, gpu_ctx, oracle):
    """Packed codes and results stay in HBM; each output NULL in turn and left untouched; a pointer 8 bytes off the
    16-byte alignment is refused.  The device buffers come from the HIP runtime the product library already holds, as in
    tests/test_pairwise_windows.py::test_windows_device_resident_entry."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    n, sites = 21, 50_001
    status, pmax, codes = _random(4, n, sites)
    packed = abn.pack_codes(codes)
    stride = packed.shape[1]
    rng = np.random.default_rng(4)
    W = 12
    begin = rng.integers(0, sites - 40_000, size=W).astype(np.int64)
    lens = rng.integers(0, 40_000, size=W)
    lens[0], begin[1], lens[1] = 0, sites - 9000, 9000        # an empty window; one to the last site of the last row
    assert lens.max() > PACKED_CHUNK_SITES > lens.min()       # chunked and direct jobs in one call
    end = begin + lens
    nout = W * (n * (n - 1) // 2)
    want = gpu_ctx.pairwise_divergence_windows_packed(packed, sites, begin, end)
    _check_against_oracle(oracle, want, status, pmax, begin, end)
    bufs = [C.c_void_p() for _ in range(4)]
    for ptr, size in zip(bufs, (packed.nbytes + 64, 8 * nout, 8 * nout, 8 * nout)):
        assert hip.hipMalloc(C.byref(ptr), size) == 0
    try:
        assert bufs[0].value % 16 == 0
        assert hip.hipMemcpy(bufs[0], packed.ctypes.data, packed.nbytes, 1) == 0
        for skip in (None, 0, 1, 2):                          # all three outputs; then each of them NULL in turn
            for ptr in bufs[1:]:
                assert hip.hipMemset(ptr, 7, 8 * nout) == 0
            ptrs = [0 if k == skip else bufs[1 + k].value for k in range(3)]
            ms = gpu_ctx.pairwise_divergence_windows_packed_dev(bufs[0].value, n, sites, stride, begin, end, *ptrs)
            assert ms > 0
            for k in range(3):
                host = np.zeros(nout, dtype=np.float64 if k == 2 else np.uint64)
                assert hip.hipMemcpy(host.ctypes.data, bufs[1 + k], 8 * nout, 2) == 0
                if k == skip:
                    assert np.all(host.view(np.uint8) == 7)   # untouched
                else:
                    assert np.array_equal(host, want[k].reshape(-1), equal_nan=(k == 2))
        with pytest.raises(abn.AbnError) as err:              # refused before anything is read
            gpu_ctx.pairwise_divergence_windows_packed_dev(bufs[0].value + 8, n, sites, stride, begin, end,
                                                           bufs[1].value, bufs[2].value, bufs[3].value)
        assert err.value.status == INVALID
    finally:
        for ptr in bufs:
            hip.hipFree(ptr)


def test_packed_windows_arguments(abn, gpu_ctx):
    sites = 300
    packed = abn.pack_codes(np.zeros((3, sites), dtype=np.uint8))
    assert packed.shape == (3, 128)
    for b, e in (([5], [4]), ([0], [sites + 1]), ([-1], [10]), ([0, 50], [10, 49]), ([0], [512])):
        with pytest.raises(abn.AbnError) as err:
            gpu_ctx.pairwise_divergence_windows_packed(packed, sites, b, e)
        assert err.value.status == INVALID
    i64p, u8p, u64p = C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    zero, ten = np.zeros(1, dtype=np.int64), np.full(1, 10, dtype=np.int64)
    out = np.full(8, 7, dtype=np.uint64)
    fn = gpu_ctx._L.abn_pairwise_divergence_windows_packed

    def call(p=packed.ctypes.data_as(u8p), n=3, L=sites, stride=128, b=zero.ctypes.data_as(i64p),
             e=ten.ctypes.data_as(i64p), W=1):
        return fn(gpu_ctx._h, p, n, L, stride, b, e, W, out.ctypes.data_as(u64p), None, None)

    assert call() == 0 and np.all(out[:3] == 0) and np.all(out[3:] == 7)
    out[:] = 7
    # what the one-matrix packed entry refuses
    assert call(p=None) == INVALID and call(n=0) == INVALID and call(n=-2) == INVALID and call(L=-1) == INVALID
    assert call(stride=96) == INVALID and call(stride=64) == INVALID and call(stride=-64) == INVALID
    assert call(n=65536) == INVALID
    # the windows
    assert call(W=-1) == INVALID and call(b=None) == INVALID and call(e=None) == INVALID
    # a window so long that one of its chunks would reach 2^30 sites (nothing is read or allocated before the refusal)
    huge = np.full(1, MAX_JOBS << 30, dtype=np.int64)
    assert call(L=int(huge[0]), stride=int(huge[0]) // 4, e=huge.ctypes.data_as(i64p)) == INVALID
    assert np.all(out == 7)
    # ABN_OK and nothing written
    assert call(W=0) == 0 and call(W=0, b=None, e=None) == 0 and call(n=1) == 0
    assert np.all(out == 7)
    d, b, v = gpu_ctx.pairwise_divergence_windows_packed(packed, sites, [], [])
    assert d.shape == (0, 3) and b.shape == (0, 3) and v.shape == (0, 3)
    d, b, v = gpu_ctx.pairwise_divergence_windows_packed(packed[:1], sites, [0, 10], [10, 20])   # one sample: no pairs
    assert d.shape == (2, 0) and v.size == 0


def test_build_many_scans_packed_codes(abn, gpu_ctx, tmp_path):
    """Pedigree::build_many(gpu) — packed straight from the site records, one abn_pairwise_divergence_windows_packed
    call per batch — against Pedigree::build's host loop per window, bit for bit; the call counter rises."""
    from pathlib import Path

    from _build_many import build_each, build_many, hostlib, write_windows

    L = hostlib()
    L.abh_packed_windows_scan_calls.restype = C.c_longlong
    lists = write_windows(tmp_path, Path(__file__).resolve().parent / "golden")
    before = L.abh_packed_windows_scan_calls()
    many = build_many(L, lists, gpu=True)
    assert L.abh_packed_windows_scan_calls() == before + 2       # the four-sample windows; the three-sample window
    each = build_each(L, lists)
    assert [m[0] for m in many] == [6, 6, -1, 3, 6, 6, 6]
    assert b"could not read nodelist" in many[2][3]
    for m, e in zip(many, each):
        assert m[0] == e[0] and m[3] == e[3]
        if m[0] >= 0:
            assert m[1].tobytes() == e[1].tobytes() and m[2] == e[2]
    assert len({m[1].tobytes() for m in many if m[0] == 6}) == 5      # the windows do differ
