"""abn_pairwise_divergence_packed{,_dev} — DMatrix::from (src/pedigree.rs:210-261) on 2-bit packed codes — against the
oracle and against the byte scan on the same sites.  The sums are integers and D is one f64 division: every comparison
is exact (np.array_equal on diff and both, bit equality on dvalue with the NaN positions equal).  Shapes sit on the
edges of the format and of the job geometry: the 16-sample block, the 64-sample group, the 16-site field group, the
256-site super-step, the chunks of a super-pair, the job slab of one launch."""
import ctypes as C
import os
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
INVALID = 1  # ABN_ERR_INVALID_ARG

pytestmark = pytest.mark.gpu


def _codes(status, pmax, flt=0.99):
    return (status | np.where(pmax < flt, 0x80, 0)).astype(np.uint8)


def _random(seed, n, L, filtered=None):
    rng = np.random.default_rng(seed)
    frac = rng.uniform(0.0, 0.6) if filtered is None else filtered
    status = rng.integers(0, 3, size=(n, L), dtype=np.uint8)
    pmax = np.where(rng.random((n, L)) < frac, 0.5, 1.0)
    return status, pmax


def _same(got, want):
    """exact: integers equal, dvalue bit-equal with NaN where the reference has NaN"""
    (gd, gb, gv), (wd, wb, wv) = got, want
    assert np.array_equal(gd, wd) and np.array_equal(gb, wb)
    assert np.array_equal(np.isnan(gv), np.isnan(wv))
    ok = ~np.isnan(wv)
    assert np.array_equal(gv[ok].view(np.uint64), wv[ok].view(np.uint64))


@pytest.mark.parametrize("n,L", [(2, 1), (15, 15), (16, 16), (17, 255), (64, 256), (65, 257), (130, 4099), (15, 70_001),
                                 (130, 1), (2, 257), (17, 4099), (64, 70_001), (65, 15), (16, 255), (130, 256)])
def test_packed_against_oracle_and_byte_scan(abn, gpu_ctx, oracle, n, L):
    status, pmax = _random(1000 * n + L, n, L)
    codes = _codes(status, pmax)
    got = gpu_ctx.pairwise_divergence_packed(abn.pack_codes(codes), L)
    _same(got, oracle.pairwise_divergence(status, pmax, 0.99))
    _same(got, gpu_ctx.pairwise_divergence(codes))


def test_every_state_pair_operand_order_and_field_position(abn, gpu_ctx, oracle):
    """Every ordered pair of the four states {U, I, M, filtered} on two samples of DIFFERENT blocks and groups, at every
    one of the 16 positions of a field group, in known and unequal counts; the other 15 positions of those groups are
    filtered for sample a, so the pair's sums are known by hand: a wrong bit position, a swapped table half or a table
    entry for 3 that is not zero changes them."""
    n, a, b = 150, 3, 141
    states = [0, 1, 2, 0x80]
    rng = np.random.default_rng(7)
    groups = []                                          # (position, state of a, state of b), repeated
    for pos in range(16):
        for ia in range(4):
            for ib in range(4):
                groups += [(pos, ia, ib)] * ((pos + 4 * ia + ib) % 5 + 1)
    L = 16 * len(groups)
    codes = np.array([0, 1, 2, 0x80, 0x81, 0x82], dtype=np.uint8)[rng.integers(0, 6, size=(n, L))]
    codes[a] = 0x80
    want_both = want_diff = 0
    for g, (pos, ia, ib) in enumerate(groups):
        codes[a, 16 * g + pos] = states[ia]
        codes[b, 16 * g + pos] = states[ib]
        if ia < 3 and ib < 3:
            want_both += 1
            want_diff += abs(ia - ib)
    got = gpu_ctx.pairwise_divergence_packed(abn.pack_codes(codes), L)
    p = a * n - a * (a + 1) // 2 + (b - a - 1)
    assert int(got[1][p]) == want_both and int(got[0][p]) == want_diff
    status, pmax = codes & 3, np.where(codes & 0x80, 0.5, 1.0)
    _same(got, oracle.pairwise_divergence(status, pmax, 0.99))
    _same(got, gpu_ctx.pairwise_divergence(codes))
    # ... and with the operands swapped (a in the later group)
    codes[[a, b]] = codes[[b, a]]
    got = gpu_ctx.pairwise_divergence_packed(abn.pack_codes(codes), L)
    assert int(got[1][p]) == want_both and int(got[0][p]) == want_diff
    _same(got, gpu_ctx.pairwise_divergence(codes))


def test_filtered_samples_and_equal_samples(abn, gpu_ctx, oracle):
    n, L = 21, 700
    status, pmax = _random(3, n, L, filtered=0.2)
    pmax[[2, 17]] = 0.1                                   # whole samples filtered: both = 0, 0 / 0 = NaN
    status[5] = status[19]                                # equal samples: diff = 0 on the sites both keep
    got = gpu_ctx.pairwise_divergence_packed(abn.pack_codes(_codes(status, pmax)), L)
    _same(got, oracle.pairwise_divergence(status, pmax, 0.99))
    pair = lambda i, j: i * n - i * (i + 1) // 2 + (j - i - 1)
    for i in range(n):
        for j in range(i + 1, n):
            if i in (2, 17) or j in (2, 17):
                assert got[1][pair(i, j)] == 0 and got[0][pair(i, j)] == 0 and np.isnan(got[2][pair(i, j)])
    assert got[0][pair(5, 19)] == 0 and got[1][pair(5, 19)] > 0 and got[2][pair(5, 19)] == 0.0


def test_degenerate(abn, gpu_ctx):
    d, b, v = gpu_ctx.pairwise_divergence_packed(abn.pack_codes(np.zeros((1, 10), dtype=np.uint8)), 10)   # no pairs
    assert d.size == 0
    d, b, v = gpu_ctx.pairwise_divergence_packed(abn.pack_codes(np.zeros((3, 0), dtype=np.uint8)), 0)     # no sites
    assert d.size == 3 and np.all(b == 0) and np.all(d == 0) and np.all(np.isnan(v))
    d, b, v = gpu_ctx.pairwise_divergence_packed(np.full((3, 64), 0xFF, dtype=np.uint8), 0)   # ... with room in the rows
    assert np.all(b == 0) and np.all(d == 0) and np.all(np.isnan(v))


def test_refusals(abn, gpu_ctx):
    L = abn.load_library()
    packed = abn.pack_codes(np.zeros((3, 300), dtype=np.uint8))
    out = np.zeros(3, dtype=np.uint64)
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    call = lambda ptr, n, sites, stride: L.abn_pairwise_divergence_packed(gpu_ctx._h, ptr, n, sites, stride,
                                                                          out.ctypes.data_as(u64p), None, None)
    assert call(packed.ctypes.data_as(u8p), 3, 300, 128) == 0
    assert call(None, 3, 300, 128) == INVALID
    assert call(packed.ctypes.data_as(u8p), 3, 300, 64) == INVALID          # below abn_packed_row_stride(300)
    assert call(packed.ctypes.data_as(u8p), 3, 300, 160) == INVALID         # not a multiple of 64
    assert call(packed.ctypes.data_as(u8p), 65536, 300, 128) == INVALID     # too many samples (refused before any read)


def test_larger_stride_same_result(abn, gpu_ctx):
    n, L = 33, 1500
    status, pmax = _random(11, n, L)
    codes = _codes(status, pmax)
    tight = gpu_ctx.pairwise_divergence_packed(abn.pack_codes(codes), L)
    for stride in (abn.packed_row_stride(L) + 64, 1024):
        _same(gpu_ctx.pairwise_divergence_packed(abn.pack_codes(codes, row_stride=stride), L), tight)
    _same(tight, gpu_ctx.pairwise_divergence(codes))


# ---- the launch policy of csrc/abn_pairwise.hip (pairwise_family) as a model: jobs of one family of super-pairs
def _max_jobs():
    src = (ROOT / "alphabeta_rs_amd" / "csrc" / "abn_pairwise.hip").read_text()
    return int(re.search(r"kPmxMaxJobs = (\d+);", src).group(1))


def _family_jobs(cus, nsp, L, cu_jobs=1):
    steps = (L + 255) // 256                               # super-steps of a row
    nchunks = max(1, (cus * cu_jobs + nsp - 1) // nsp)
    nchunks = min(nchunks, max(1, steps // 16))            # four super-steps per wavefront at least
    nchunks = max(nchunks, (L >> 30) + 1)
    return nsp * nchunks


def test_more_jobs_than_one_launch_holds(abn, gpu_ctx, oracle):
    """The smallest n x L whose off-diagonal family needs two slabs: with as many super-pairs as CUs or more a super-pair
    is one chunk, so the jobs are the super-pairs and 129 groups (8193 samples: 8256 pairs of groups) are the first to
    exceed kPmxMaxJobs; L = 17 keeps it one super-step (L does not add jobs here).  The second slab reuses the partial
    rows of the first in stream order."""
    cus = gpu_ctx.device_info()["compute_units"]
    n, L = 128 * 64 + 1, 17
    g = (n + 63) // 64
    assert _family_jobs(cus, g * (g - 1) // 2, L) > _max_jobs()              # this shape crosses the slab ...
    assert _family_jobs(cus, (g - 1) * (g - 2) // 2, L) <= _max_jobs()       # ... and one group fewer does not
    assert _family_jobs(cus, g, L, cu_jobs=2) <= _max_jobs()
    status, pmax = _random(99, n, L, filtered=0.3)
    got = gpu_ctx.pairwise_divergence_packed(abn.pack_codes(_codes(status, pmax)), L)
    _same(got, oracle.pairwise_divergence(status, pmax, 0.99))


def test_several_chunks_per_super_pair_in_the_model(gpu_ctx):
    """the parametrised shapes above do cut super-pairs into several chunks (70 001 sites: 274 super-steps)"""
    cus = gpu_ctx.device_info()["compute_units"]
    assert _family_jobs(cus, 1, 70_001) == 17 and _family_jobs(cus, 3, 4099) == 3 and _family_jobs(cus, 1, 4099) == 1


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")        # the HIP runtime the product library already holds
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


@pytest.mark.parametrize("n,L", [(15, 70_001), (65, 4099)])
def test_device_resident_entry(abn, gpu_ctx, hip, n, L):
    status, pmax = _random(n + L, n, L)
    codes = _codes(status, pmax)
    packed = abn.pack_codes(codes)
    stride = packed.shape[1]
    npairs = n * (n - 1) // 2
    bufs = [C.c_void_p() for _ in range(4)]
    for ptr, size in zip(bufs, (packed.nbytes + 16, 8 * npairs, 8 * npairs, 8 * npairs)):
        assert hip.hipMalloc(C.byref(ptr), size) == 0
    t, d, b, v = bufs
    try:
        assert hip.hipMemcpy(t, packed.ctypes.data, packed.nbytes, 1) == 0
        ms = gpu_ctx.pairwise_divergence_packed_dev(t.value, n, L, stride, d.value, b.value, v.value)
        assert ms > 0
        dd, db, dv = np.zeros(npairs, np.uint64), np.zeros(npairs, np.uint64), np.zeros(npairs)
        for host, dev in ((dd, d), (db, b), (dv, v)):
            assert hip.hipMemcpy(host.ctypes.data, dev, 8 * npairs, 2) == 0
        want = gpu_ctx.pairwise_divergence_packed(packed, L)
        _same((dd, db, dv), want)
        _same(want, gpu_ctx.pairwise_divergence(codes))
        # NULL outputs: only what is asked for is written
        zeros = np.zeros(npairs, np.uint64)
        assert hip.hipMemcpy(d, zeros.ctypes.data, 8 * npairs, 1) == 0
        assert gpu_ctx.pairwise_divergence_packed_dev(t.value, n, L, stride, 0, b.value, 0) > 0
        assert gpu_ctx.pairwise_divergence_packed_dev(t.value, n, L, stride) > 0
        assert hip.hipMemcpy(dd.ctypes.data, d, 8 * npairs, 2) == 0 and not dd.any()
        assert hip.hipMemcpy(db.ctypes.data, b, 8 * npairs, 2) == 0 and np.array_equal(db, want[1])
        # a device pointer that is not 16-byte aligned is refused
        with pytest.raises(abn.AbnError) as e:
            gpu_ctx.pairwise_divergence_packed_dev(t.value + 8, n, L, stride, d.value, b.value, v.value)
        assert e.value.status == INVALID
    finally:
        for ptr in bufs:
            hip.hipFree(ptr)


def test_pedigree_build_takes_the_packed_entry(abn, gpu_ctx, golden, tmp_path):
    """Pedigree::build with gpu_pairwise (what the `alphabeta` CLI calls) on the bundled methylomes: the pedigree file is
    byte-equal to data/pedigree_generated.txt, and the scan went through abn_pairwise_divergence_packed."""
    from alphabeta_rs_amd import build as B

    B.build_host()
    H = C.CDLL(str(B.PEDIGREE_LIB))
    H.abh_pedigree_build_gpu.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.c_char_p, C.POINTER(C.c_double), C.c_int,
                                         C.POINTER(C.c_double), C.c_char_p, C.c_int]
    H.abh_packed_scan_calls.restype = C.c_longlong
    before = H.abh_packed_scan_calls()
    out = tmp_path / "pedigree.txt"
    rows, p0, err = np.zeros((64, 4)), C.c_double(), C.create_string_buffer(256)
    cwd = os.getcwd()
    os.chdir(GOLDEN)  # the nodelist names ./data/methylome/*.txt relative to the working directory
    try:
        n = H.abh_pedigree_build_gpu(b"./data/nodelist.txt", b"./data/edgelist.txt", 0.99, str(out).encode(),
                                     rows.ctypes.data_as(C.POINTER(C.c_double)), 64, C.byref(p0), err, 256)
    finally:
        os.chdir(cwd)
    assert n == 6, err.value
    assert H.abh_packed_scan_calls() == before + 1
    assert out.read_bytes() == (GOLDEN / "pedigree_generated.txt").read_bytes()
    assert np.array_equal(rows[:n], golden["generated"]) and p0.value == golden["p0uu_generated"]
