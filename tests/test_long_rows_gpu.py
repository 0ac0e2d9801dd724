"""The packed and byte scans, the census and the simulator at genome-scale rows: past 2^26 and 2^28 sites, where a window's
chunks grow beyond their usual size (pairwise_windows_chunks, csrc/abn_pairwise.hip), and past 2^31 sites, 2^32 sites, 2^32
bytes and counts of 2^32.  The rows are never built on the host: a period of 12 316 bytes is doubled over the buffer by
device-to-device copies, and the expected integers come from the prefix counts of tests/_long_rows_model.py (held against
brute force by tests/test_long_rows_cpu.py); the simulator is compared at slices of its rows with the slice forms of
tests/_sim_model.py and _sim_obs_model.py.  Every comparison is exact; every test first asserts, from its own inputs and
from constants read out of the sources, that the path it is there for is reached."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import _long_rows_model as LR
import _sim_model as SM
import _sim_obs_model as OM
from alphabeta_rs_amd import census
from alphabeta_rs_amd import simulate as S

pytestmark = pytest.mark.gpu
CSRC = Path(__file__).resolve().parent.parent / "alphabeta_rs_amd" / "csrc"
H2D, D2H, D2D = 1, 2, 3
SEED = 0x9E3779B97F4A7C15
RATES = (0.1, 0.2, 0.7, 0.3)     # the fast rates of tests/test_sim_gpu.py


def _constant(header, name):
    return int(re.search(name + r" = (\d+);", (CSRC / header).read_text()).group(1))


MAX_JOBS = _constant("abn_pairwise.hip", "kPmxMaxJobs")                        # jobs per launch of the divergence scans ...
CENSUS_MAX_JOBS = MAX_JOBS                                                     # ... and of the census, which takes their cuts
TRANS_MAX_JOBS = _constant("abn_pairwise_transitions.hpp", "kTransMaxJobs")    # ... of the transitions scan
PACKED_CHUNK = _constant("abn_packed_mask.hpp", "kPmxWinPackedChunkSites")     # sites per job of a packed window
BYTE_CHUNK = _constant("abn_pairwise_windows.hpp", "kPmxWinChunkSites")        # ... of a byte window
STEP = _constant("abn_packed_mask.hpp", "kPackedStepSites")


def test_the_constants_are_the_ones_the_sizes_below_were_chosen_for():
    assert (MAX_JOBS, TRANS_MAX_JOBS, PACKED_CHUNK, BYTE_CHUNK, STEP) == (8192, 2048, 32768, 8192, 256)


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")        # the HIP runtime the product library already holds
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    h.hipFree.argtypes = [C.c_void_p]
    h.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    h.hipDeviceSynchronize.argtypes = []
    return h


class Device:
    """buffers of one test: freed by close(); a failed hipMalloc fails the test"""

    def __init__(self, hip):
        self.hip, self.ptrs, self.bytes = hip, [], 0
        free, total = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        self.free0 = self.low = free.value

    def alloc(self, size):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(int(size), 4)) == 0, f"hipMalloc of {size} bytes"
        self.ptrs.append(p)
        self.bytes += int(size)
        assert self.bytes <= 6 << 30
        return p.value

    def note(self):
        """the least free device memory seen: the scans' own rows of partial sums lie beside the test's buffers"""
        free, total = C.c_size_t(), C.c_size_t()
        assert self.hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        self.low = min(self.low, free.value)

    def close(self, name=""):
        self.note()
        print(f"[long rows] {name}: {self.bytes / 2**30:.3f} GiB of buffers, {(self.free0 - self.low) / 2**30:.3f} GiB in use at most "
              "between calls")
        for p in self.ptrs:
            self.hip.hipFree(p)

    def put(self, at, array):
        array = np.ascontiguousarray(array)
        assert self.hip.hipMemcpy(at, array.ctypes.data, array.nbytes, H2D) == 0

    def get(self, at, shape, dtype):
        out = np.zeros(shape, dtype=dtype)
        assert self.hip.hipMemcpy(out.ctypes.data, at, out.nbytes, D2H) == 0
        return out

    def set(self, at, value, size):
        assert self.hip.hipMemset(at, value, size) == 0 and self.hip.hipDeviceSynchronize() == 0

    def fill_stream(self, at, per, size):
        """the period repeated from byte 0 over [at, at + size): one upload, then copies of what lies there already, each
        over a range that does not overlap its source and begins at a whole number of periods"""
        have = min(LR.P, size)
        self.put(at, per[:have])
        while have < size:
            assert have % LR.P == 0
            count = min(have, size - have)
            assert self.hip.hipMemcpy(at + have, at, count, D2D) == 0
            have += count
        assert self.hip.hipDeviceSynchronize() == 0

    def patch_tails(self, at, view, restore=False):
        """the padding of every packed row as the whole-matrix scan wants it (restore: the stream's own bytes again)"""
        for r in range(view.n):
            self.put(at + view.tail_offset(r), view.stream(view.tail_offset(r), 64) if restore else view.tail(r))


class Outputs:
    """device outputs of `count` 8-byte entries each, set to a pattern before a call and read after it"""

    def __init__(self, dev, count, names=("diff", "both", "dvalue")):
        self.dev, self.count = dev, count
        self.ptr = {k: dev.alloc(8 * count) for k in names}

    def reset(self):
        for p in self.ptr.values():
            self.dev.set(p, 7, 8 * self.count)

    def read(self, name, shape, dtype=np.uint64):
        out = self.dev.get(self.ptr[name], (self.count,), dtype)
        used = int(np.prod(shape))
        assert np.all(out[used:].view(np.uint8) == 7)                       # nothing behind the entries that were asked for
        return out[:used].reshape(shape)

    def untouched(self, name):
        return bool(np.all(self.dev.get(self.ptr[name], (8 * self.count,), np.uint8) == 7))


def _u64(a):
    assert np.all(np.asarray(a) >= 0)
    return np.asarray(a).astype(np.uint64)


def check_divergence_windows(out, call, view, begin, end):
    """a windows divergence entry against the model: diff, both and D; then diff alone, both and D not asked for"""
    n, W = view.n, len(begin)
    pairs = n * (n - 1) // 2
    both, diff = LR.folds(view.tables(begin, end))
    out.reset()
    assert call(out.ptr["diff"], out.ptr["both"], out.ptr["dvalue"]) > 0
    got_diff, got_both = out.read("diff", (W, pairs)), out.read("both", (W, pairs))
    got_d = out.read("dvalue", (W, pairs), np.float64)
    for w in range(W):
        assert np.array_equal(got_both[w], _u64(both[w])) and np.array_equal(got_diff[w], _u64(diff[w])), (w, begin[w], end[w])
        assert np.array_equal(got_d[w], LR.dvalue(diff[w], both[w]), equal_nan=True), (w, begin[w], end[w])
    out.reset()
    assert call(out.ptr["diff"], 0, 0) > 0
    assert np.array_equal(out.read("diff", (W, pairs)), _u64(diff)) and out.untouched("both") and out.untouched("dvalue")
    return diff, both


def check_transitions_windows(gpu_ctx, out, at, view, begin, end):
    n, W = view.n, len(begin)
    pairs = n * (n - 1) // 2
    want = view.tables(begin, end)
    out.reset()
    assert gpu_ctx.pairwise_transitions_windows_packed_dev(at, n, view.L, view.stride, begin, end, out.ptr["table"]) > 0
    got = out.read("table", (W, pairs, 3, 3))
    for w in range(W):
        assert np.array_equal(got[w], _u64(want[w])), (w, begin[w], end[w])
    return want


def check_census_windows(gpu_ctx, out, at, view, begin, end):
    want = view.census(begin, end)
    out.reset()
    assert census.census_windows_dev(gpu_ctx, at, view.n, view.L, view.stride, begin, end, out.ptr["counts"]) > 0
    got = out.read("counts", (len(begin), view.n, 3))
    for w in range(len(begin)):
        assert np.array_equal(got[w], _u64(want[w])), (w, begin[w], end[w])
    return want


def among_short_ones(L, longs):
    """the long windows, each between short ones of under 1000 sites: at the front, behind the long one's begin, at the
    row's end"""
    begin, end = [], []
    for k, (b, e) in enumerate(longs):
        begin += [3 + 17 * k, b, b + 4099 + k, L - 700 - k]
        end += [3 + 17 * k + 600 + k, e, b + 4099 + k + 999, L - k]
    return np.array(begin, dtype=np.int64), np.array(end, dtype=np.int64)


def windows_at_the_boundary(L, sites, max_jobs, align):
    """[(begin, end)] whose span — from the begin rounded down to `align` — is max_jobs jobs of `sites` exactly (the most
    that is not grown: the window fills a launch alone) and one site more (grown), the begin at a cut and 5 sites behind"""
    full = max_jobs * sites
    base = 2 * 256 if align > 1 else 4097                                   # byte windows: begins at odd bytes
    lead = 5 if align > 1 else 2
    from_ = base if align > 1 else base + lead                              # where the span of the last two is counted from
    longs = [(base, base + full), (base, base + full + 1), (base + lead, from_ + full), (base + lead, from_ + full + 1)]
    for k, (b, e) in enumerate(longs):
        ch, grown, jobs = LR.chunk_of(b, e, sites, align, max_jobs)
        assert e <= L and grown == (k % 2 == 1)
        assert (ch, jobs) == ((sites, max_jobs) if not grown else (sites + max(align, 128), (full + 1 + ch - 1) // ch))
        assert max_jobs // 2 < jobs <= max_jobs
    assert {b % 256 for b, _ in longs} == ({0, 5} if align > 1 else {1, 3})
    return longs


# ---------------------------------------------------------------- 1. grown chunks of packed windows, both sides of the boundary
@pytest.mark.parametrize("n,L", [(3, (1 << 28) + 3 * 256 + 7), (17, (1 << 26) + 3 * 256 + 7), (65, (1 << 26) + 3 * 256 + 7)])
def test_grown_chunks_of_packed_windows(gpu_ctx, hip, n, L):
    """n = 3: one 16-block; 17: two; 65: two groups — an off-diagonal super-pair and a one-block diagonal one.  The
    transitions scan grows a window's chunks past 2048 x 32 768 = 2^26 sites, the divergence scan and the census (which
    takes that scan's cuts) past 8192 x 32 768 = 2^28: the rows of 2^26 sites hold only the former"""
    view = LR.View(LR.period(n, "packed"), "packed", n, L)
    pairs = n * (n - 1) // 2
    trans = windows_at_the_boundary(L, PACKED_CHUNK, TRANS_MAX_JOBS, STEP)
    assert trans[0][1] - trans[0][0] == 1 << 26
    dev = Device(hip)
    try:
        at = dev.alloc(n * view.stride)
        assert at % 16 == 0
        dev.fill_stream(at, view.per, n * view.stride)
        dev.patch_tails(at, view)
        begin, end = among_short_ones(L, trans)
        out = Outputs(dev, 9 * pairs * len(begin) + 3, ("table", "counts", "diff", "both", "dvalue"))
        table = check_transitions_windows(gpu_ctx, out, at, view, begin, end)
        dev.note()
        assert table[1].sum() > 0 and np.all(table[0] <= 999)
        # the whole matrix is the one window [0, L): grown
        ch, grown, jobs = LR.chunk_of(0, L, PACKED_CHUNK, STEP, TRANS_MAX_JOBS)
        assert grown and ch > PACKED_CHUNK and ch % STEP == 0 and jobs <= TRANS_MAX_JOBS
        assert ch == PACKED_CHUNK + STEP or L > 1 << 28
        out.reset()
        assert gpu_ctx.pairwise_transitions_packed_dev(at, n, L, view.stride, out.ptr["table"]) > 0
        assert np.array_equal(out.read("table", (pairs, 3, 3)), _u64(view.tables([0], [L])[0]))
        dev.note()
        if n <= 17:
            # the census at the same windows: its launch holds 8192 jobs, so they are cut at 32 768 sites, not grown
            assert all(not LR.chunk_of(b, e, PACKED_CHUNK, STEP, CENSUS_MAX_JOBS)[1] for b, e in trans)
            check_census_windows(gpu_ctx, out, at, view, begin, end)
            dev.note()
        if L > MAX_JOBS * PACKED_CHUNK:
            longs = windows_at_the_boundary(L, PACKED_CHUNK, MAX_JOBS, STEP)
            assert longs[0][1] - longs[0][0] == 1 << 28
            begin, end = among_short_ones(L, longs)
            check_divergence_windows(
                out, lambda d, b, v: gpu_ctx.pairwise_divergence_windows_packed_dev(at, n, L, view.stride, begin, end, d, b, v),
                view, begin, end)
            dev.note()
            check_census_windows(gpu_ctx, out, at, view, begin, end)           # grown here
            dev.note()
            check_transitions_windows(gpu_ctx, out, at, view, begin, end)      # and chunks of about 2^17 sites
    finally:
        dev.close(f"grown packed windows, n = {n}")


# ---------------------------------------------------------------- 2. grown chunks of byte windows
@pytest.mark.parametrize("L", [(1 << 26) + 8192 + 5, (1 << 26) + 8192 + 8], ids=["unaligned", "aligned"])
def test_grown_chunks_of_byte_windows(gpu_ctx, hip, L):
    """windows of 8192 x 8192 sites (a launch's jobs exactly) and one site more (grown), from odd bytes.  A begin that is no
    multiple of 4 takes the loader of any alignment whatever the row length, so the row length that is a multiple of 4 is
    scanned once more with every begin on a dword: the dword loader on grown chunks"""
    n = 3
    view = LR.View(LR.period(L % 100, "bytes"), "bytes", n, L)
    longs = windows_at_the_boundary(L, BYTE_CHUNK, MAX_JOBS, 1)
    assert longs[0][1] - longs[0][0] == 1 << 26 and all(b % 2 == 1 for b, _ in longs)
    dev = Device(hip)
    try:
        at = dev.alloc(n * L)
        dev.fill_stream(at, view.per, n * L)
        begin, end = among_short_ones(L, longs)
        out = Outputs(dev, 3 * len(begin) + 3)
        call = lambda d, b, v: gpu_ctx.pairwise_divergence_windows_dev(at, n, L, begin, end, d, b, v)
        assert not (L % 4 == 0 and at % 4 == 0 and np.all(begin % 4 == 0))                  # the loader of any alignment
        check_divergence_windows(out, call, view, begin, end)
        if L % 4 == 0:
            # the dword loader: the row length, the pointer and every begin a multiple of 4
            longs4 = [(4096, 4096 + (1 << 26)), (4096, 4096 + (1 << 26) + 1), (8, L)]
            assert [LR.chunk_of(b, e, BYTE_CHUNK, 1, MAX_JOBS)[:2] for b, e in longs4] == \
                [(BYTE_CHUNK, False), (BYTE_CHUNK + 128, True), (BYTE_CHUNK + 128, True)]
            begin, end = among_short_ones(L, longs4)
            begin = begin // 4 * 4
            assert at % 4 == 0 and np.all(begin % 4 == 0) and np.all(begin <= end) and end.max() == L
            check_divergence_windows(out, call, view, begin, end)
    finally:
        dev.close(f"grown byte windows, L = {L}")


# ---------------------------------------------------------------- 3. past 32 bits, packed
def test_packed_rows_past_32_bits(gpu_ctx, hip):
    """three rows of 5 x 2^30 + 12 345 sites, 64 bytes apart and then tight: every pair's sums and every sample's largest
    census count need more than 32 bits, and windows lie across the sites 2^31 and 2^32"""
    n, L = 3, 5 * (1 << 30) + 12_345
    per = LR.period(32, "packed")
    tight = LR.View(per, "packed", n, L)
    loose = LR.View(per, "packed", n, L, tight.least + 64)
    assert L > 1 << 32 and tight.stride > 1 << 30
    for view in (tight, loose):
        both, diff = LR.folds(view.tables([0], [L])[0])
        assert both.min() >= 1 << 32 and diff.min() >= 1 << 32
        assert view.census([0], [L])[0].max(axis=1).min() > 1 << 31
    windows = [(0, L), ((1 << 31) - 70_001, (1 << 31) + 33_003), ((1 << 32) - 12_345, (1 << 32) + 40_000),
               ((1 << 32) + 5, (1 << 32) + 305), (L, L), (L - 7, L), (17, 900)]
    begin, end = (np.array(x, dtype=np.int64) for x in zip(*windows))
    assert LR.chunk_of(0, L, PACKED_CHUNK, STEP, MAX_JOBS)[1] and LR.chunk_of(0, L, PACKED_CHUNK, STEP, TRANS_MAX_JOBS)[0] < 1 << 30
    pairs = 3
    dev = Device(hip)
    try:
        at = dev.alloc(n * loose.stride)
        assert at % 16 == 0
        dev.fill_stream(at, per, n * loose.stride)
        out = Outputs(dev, 9 * pairs * len(begin) + 3, ("table", "counts", "diff", "both", "dvalue"))
        for view in (loose, tight):
            dev.patch_tails(at, view)
            want = view.tables([0], [L])[0]
            both, diff = LR.folds(want)
            out.reset()
            assert gpu_ctx.pairwise_divergence_packed_dev(at, n, L, view.stride, out.ptr["diff"], out.ptr["both"], out.ptr["dvalue"]) > 0
            got_diff, got_both = out.read("diff", (pairs,)), out.read("both", (pairs,))
            assert np.array_equal(got_diff, _u64(diff)) and np.array_equal(got_both, _u64(both))
            assert np.array_equal(out.read("dvalue", (pairs,), np.float64), LR.dvalue(diff, both))
            out.reset()
            assert gpu_ctx.pairwise_divergence_packed_dev(at, n, L, view.stride, 0, out.ptr["both"], 0) > 0
            assert np.array_equal(out.read("both", (pairs,)), _u64(both)) and out.untouched("diff") and out.untouched("dvalue")
            out.reset()
            assert gpu_ctx.pairwise_transitions_packed_dev(at, n, L, view.stride, out.ptr["table"]) > 0
            table = out.read("table", (pairs, 3, 3))
            assert np.array_equal(table, _u64(want))
            tb, td = table.sum(axis=(-1, -2)), (table * _u64(LR.ABS)).sum(axis=(-1, -2))
            assert np.array_equal(tb, got_both) and np.array_equal(td, got_diff)            # its folds are the divergence's
            check_census_windows(gpu_ctx, out, at, view, begin[:1], end[:1])
            dev.note()
            if view is tight:
                check_divergence_windows(
                    out, lambda d, b, v: gpu_ctx.pairwise_divergence_windows_packed_dev(at, n, L, view.stride, begin, end, d, b, v),
                    view, begin, end)
                dev.note()
                check_transitions_windows(gpu_ctx, out, at, view, begin, end)
                dev.note()
                cen = check_census_windows(gpu_ctx, out, at, view, begin, end)
                assert not cen[4].any() and cen[5].sum(axis=1).max() <= 7
            dev.patch_tails(at, view, restore=True)
    finally:
        dev.close("packed rows past 32 bits")


# ---------------------------------------------------------------- 4. past 32 bits, byte codes
def test_byte_rows_past_32_bits(gpu_ctx, hip):
    """five rows of 2^30 + 37 bytes in a buffer of exactly that size — the last row's ragged end is the buffer's end — and,
    in the same buffer, of 2^30 + 8: row 4 begins behind byte 2^32 in both"""
    n = 5
    lengths = [(1 << 30) + 37, (1 << 30) + 8]
    per = LR.period(64, "bytes")
    dev = Device(hip)
    try:
        size = n * lengths[0]                                               # exactly the rows of the longer view
        at = dev.alloc(size)
        dev.fill_stream(at, per, size)
        out = Outputs(dev, 10 * 10 + 3)
        for L in lengths:
            view = LR.View(per, "bytes", n, L)
            assert 4 * L > 1 << 32                                          # row 4 begins behind byte 2^32
            assert (L % 4 == 0 and at % 4 == 0) == (L == lengths[1])        # the loader of any alignment, then the dword one
            if L == lengths[0]:
                assert view.end_of_buffer() == size and L % 64 != 0         # the last row's ragged end is the buffer's
            both, diff = LR.folds(view.tables([0], [L])[0])
            out.reset()
            assert gpu_ctx.pairwise_divergence_dev(at, n, L, out.ptr["diff"], out.ptr["both"], out.ptr["dvalue"]) > 0
            assert np.array_equal(out.read("diff", (10,)), _u64(diff)) and np.array_equal(out.read("both", (10,)), _u64(both))
            assert np.array_equal(out.read("dvalue", (10,), np.float64), LR.dvalue(diff, both))
            out.reset()
            assert gpu_ctx.pairwise_divergence_dev(at, n, L, 0, 0, out.ptr["dvalue"]) > 0
            assert np.array_equal(out.read("dvalue", (10,), np.float64), LR.dvalue(diff, both))
            assert out.untouched("diff") and out.untouched("both")
            dev.note()
            half = 1 << 29
            windows = [(0, 3000), (4, 70_004), (half - 40_000, half + 40_004), (half + 4, half + 900), (L - 100, L), (L, L),
                       (L - 20_000 - L % 4, L)]
            if L % 4:
                windows += [(1, 4099), (half - 4099, half + 70_001)]        # begins that are no multiple of 4
            begin, end = (np.array(x, dtype=np.int64) for x in zip(*windows))
            assert bool(np.all(begin % 4 == 0)) == (L % 4 == 0)
            check_divergence_windows(out, lambda d, b, v: gpu_ctx.pairwise_divergence_windows_dev(at, n, L, begin, end, d, b, v),
                                     view, begin, end)
            dev.note()
    finally:
        dev.close("byte rows past 32 bits")


# ---------------------------------------------------------------- 5. the simulator and the observation past 32 bits
def _slices(L):
    """(first site, sites) of the slices that are compared: the front, around site 2^32, the row's end from a super-step on"""
    last = (L - 4096) // 256 * 256
    return [(0, 4096), ((1 << 32) - 2048, 4096), (last, L - last)]


def _fetch_rows(dev, at, stride, rows, first, count):
    """the bytes of the sites [first, first + count) (whole super-steps, to the row's padding) of every row"""
    nbytes = SM.row_stride(count)
    return np.stack([dev.get(at + r * stride + first // 4, (nbytes,), np.uint8) for r in range(rows)])


def test_simulation_and_observation_past_32_bits(gpu_ctx, hip):
    blocks, threads = S.launch_grid(gpu_ctx, 1 << 34)
    L = (1 << 32) + 16 * threads * blocks + 16 * 300 + 5
    assert threads == 256 and S.launch_grid(gpu_ctx, L) == (blocks, threads)       # the grid makes later trips behind 2^32
    parent, generation, emit = [-1, 0], [1, 3], [1, 1]
    thr = S.thresholds(parent, generation, *RATES)
    least = SM.row_stride(L)
    stride = least + 64
    assert least > 1 << 30 and L >> 2 > 1 << 30
    othr = OM.random_othr(np.random.default_rng(12))
    dev = Device(hip)
    try:
        at = dev.alloc(2 * stride)
        assert at % 16 == 0
        dev.set(at, 0x5A, 2 * stride)
        assert S.codes_dev(gpu_ctx, SEED, parent, thr, emit, L, at, stride) > 0
        before = []
        for first, count in _slices(L):
            got = _fetch_rows(dev, at, stride, 2, first, count)
            assert np.array_equal(got, SM.model(SEED, parent, thr.tolist(), emit, count, first=first)), first
            before.append(got)
        spare = np.stack([dev.get(at + r * stride + least, (64,), np.uint8) for r in range(2)])
        assert np.all(spare == 0x5A)
        assert np.all(OM.unpack(before[2], L - _slices(L)[2][0]) < 3) and (L % 256 != 0)
        dev.note()
        assert S.observe_dev(gpu_ctx, SEED, [0, 1], OM.as_array(othr), L, at, stride, at, stride) > 0
        for (first, count), truth in zip(_slices(L), before):
            got = _fetch_rows(dev, at, stride, 2, first, count)
            assert np.array_equal(got, OM.observe(SEED, truth, [0, 1], othr, count, first=first)), first
            assert not np.array_equal(got, truth)
        spare = np.stack([dev.get(at + r * stride + least, (64,), np.uint8) for r in range(2)])
        assert np.all(spare == 0x5A)
    finally:
        dev.close("simulation and observation past 2^32 sites")


def test_simulation_at_the_top_of_the_counter_range(gpu_ctx, hip):
    L = 1 << 34
    assert L == S.MAX_SITES and (L - 1) >> 2 == 0xFFFFFFFF                        # the last quad's counter word is all ones
    parent, emit = [-1], [1]
    thr = S.thresholds(parent, [2], *RATES)
    stride = SM.row_stride(L)
    assert stride == 1 << 32
    dev = Device(hip)
    try:
        at = dev.alloc(stride)
        counts = dev.alloc(8 * 4)
        assert S.codes_dev(gpu_ctx, SEED, parent, thr, emit, L, at, stride) > 0
        for first in (0, L - 4096):
            got = _fetch_rows(dev, at, stride, 1, first, 4096)
            assert np.array_equal(got, SM.model(SEED, parent, thr.tolist(), emit, 4096, first=first)), first
        dev.set(counts, 7, 32)
        assert census.census_windows_dev(gpu_ctx, at, 1, L, stride, [0], [L], counts) > 0
        got = dev.get(counts, (4,), np.uint64)
        assert int(got[:3].sum()) == L and got[:3].min() > 0 and got[3] == 0x0707070707070707   # no field is 3
    finally:
        dev.close("simulation of 2^34 sites")
