"""The analysis of every window's bootstrap table on the device (abn_analyze_batch*, abn_plan_analyze, abn_multi_analyze;
RawAnalysis::analyze, src/analysis.rs:50-98) against the host analysis of each window's table — abn_analyze, which is
itself pinned to the oracle's abo_analyze here — bit for bit: uint64 views, two NaN count as equal (payloads are not
part of the contract).  The device entries are never compared with each other."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, INVALID, NO_FINITE_FIT, STATE = 0, 1, 5, 6

# 8 / 9: the eight-accumulator fold and its tail; 41: 0.025 * 40 is integral (lo == hi, frac == 0); 255 / 256 / 257: around
# a workgroup's thread count
B_VALUES = (1, 2, 3, 7, 8, 9, 16, 17, 40, 41, 42, 255, 256, 257, 1000)
# the chain wavefront loads 64 values at a time and walks them in groups of eight: either side of a load, a load plus one
# group, two loads (one window is enough for these)
B_CHUNK_EDGES = (63, 64, 65, 72, 127, 128, 129)
W_VALUES = (1, 3, 70)
KINDS = ("plausible", "quantised", "special", "equal")


def _tables(kind, W, B, seed):
    rng = np.random.default_rng(seed)
    raw = rng.uniform(0.01, 0.99, (W, B, 7))
    raw[..., 0] = 10.0 ** rng.uniform(-6, -2, (W, B))       # alpha, beta log-uniform
    raw[..., 1] = 10.0 ** rng.uniform(-6, -2, (W, B))
    raw[..., 3] = rng.normal(0.0, 0.01, (W, B))              # intercept: both signs
    if kind == "plausible":
        neg = rng.random((W, B)) < 0.1                       # some fits end with a negative alpha
        raw[..., 0] = np.where(neg, -raw[..., 0], raw[..., 0])
    elif kind == "quantised":                                # five distinct values per column: ties through every digit
        for c in range(7):
            levels = raw[0, :5 if B >= 5 else B, c].copy()
            raw[..., c] = levels[rng.integers(0, len(levels), (W, B))]
    elif kind == "special":                                  # +-0.0, subnormals, one +inf and one -inf per window
        sub = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2e-308, 1e-300, -1e-300])
        for c in (1, 2, 3, 4, 5, 6):                         # (alpha stays non-zero: 0 / 0 would be a refused row)
            hit = rng.random((W, B)) < 0.6
            raw[..., c] = np.where(hit, sub[rng.integers(0, len(sub), (W, B))], raw[..., c])
        raw[:, B // 2, 4] = np.inf
        raw[:, B // 3, 5] = -np.inf
    elif kind == "equal":
        raw[...] = raw[0, 0]
    return np.ascontiguousarray(raw)


def _host(abn, oracle, raw_w):
    """abn_analyze on one window's table (status, out32); a clean table's result is the oracle's too"""
    L = abn.load_library()
    out = np.full(32, -7.0)
    dp = C.POINTER(C.c_double)
    rc = L.abn_analyze(np.ascontiguousarray(raw_w).ctypes.data_as(dp), raw_w.shape[0], out.ctypes.data_as(dp))
    if rc == OK:
        _assert_same(out, oracle.analyze(raw_w).reshape(32), "abn_analyze against the oracle")
    return rc, out


def _assert_same(got, want, what):
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    same = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), f"{what}: entries {np.flatnonzero(~same)[:8]} differ: {got[~same][:4]} != {want[~same][:4]}"


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")        # the HIP runtime the product library already holds
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


def _through_device_buffers(gpu_ctx, hip, raw, allow_failed_windows=False):
    W, B = raw.shape[:2]
    bufs = [C.c_void_p() for _ in range(3)]
    for ptr, size in zip(bufs, (raw.nbytes, W * 32 * 8, W * 4)):
        assert hip.hipMalloc(C.byref(ptr), size) == 0
    t, o, f = bufs
    try:
        assert hip.hipMemcpy(t, raw.ctypes.data, raw.nbytes, 1) == 0
        ms = gpu_ctx.analyze_batch_dev(t.value, W, B, o.value, f.value, allow_failed_windows=allow_failed_windows)
        assert ms > 0
        out, fb = np.zeros((W, 32)), np.zeros(W, dtype=np.int32)
        assert hip.hipMemcpy(out.ctypes.data, o, out.nbytes, 2) == 0 and hip.hipMemcpy(fb.ctypes.data, f, fb.nbytes, 2) == 0
        # first_bad not wanted: the same table again, out only
        assert hip.hipMemcpy(o, np.zeros((W, 32)).ctypes.data, out.nbytes, 1) == 0
        gpu_ctx.analyze_batch_dev(t.value, W, B, o.value, 0, allow_failed_windows=allow_failed_windows)
        again = np.zeros((W, 32))
        assert hip.hipMemcpy(again.ctypes.data, o, again.nbytes, 2) == 0
        return out, fb, again
    finally:
        for ptr in bufs:
            hip.hipFree(ptr)


def _check_both_entries(abn, oracle, gpu_ctx, hip, raw):
    W = raw.shape[0]
    want = np.stack([_host(abn, oracle, raw[w])[1] for w in range(W)])
    out, fb = abn.analyze_batch(gpu_ctx, raw)
    assert out.shape == (W, 32) and np.all(fb == -1)
    for w in range(W):
        _assert_same(out[w], want[w], f"abn_analyze_batch, window {w}")
    dout, dfb, again = _through_device_buffers(gpu_ctx, hip, raw)
    assert np.all(dfb == -1)
    for w in range(W):
        _assert_same(dout[w], want[w], f"abn_analyze_batch_dev, window {w}")
        _assert_same(again[w], want[w], f"abn_analyze_batch_dev without first_bad, window {w}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", B_VALUES)
def test_batch_entries_match_the_host_analysis(abn, oracle, gpu_ctx, hip, B, kind):
    for W in W_VALUES:
        raw = _tables(kind, W, B, seed=1000 * B + W)
        if kind == "special":
            assert np.isinf(raw).any() and not np.isnan(raw).any() and (B < 40 or (raw == 0).any())
        _check_both_entries(abn, oracle, gpu_ctx, hip, raw)


@pytest.mark.parametrize("B", B_CHUNK_EDGES)
def test_batch_entries_at_the_edges_of_a_load(abn, oracle, gpu_ctx, hip, B):
    for kind in KINDS:
        _check_both_entries(abn, oracle, gpu_ctx, hip, _tables(kind, 1, B, seed=77 * B))


def test_sd_of_one_bootstrap_is_nan_as_on_the_host(abn, oracle, gpu_ctx):
    raw = _tables("plausible", 3, 1, seed=5)
    out, fb = abn.analyze_batch(gpu_ctx, raw)
    assert np.all(fb == -1) and np.isnan(out[:, 8:16]).all() and not np.isnan(out[:, :8]).any()
    assert np.array_equal(out[:, 16:24], out[:, 24:32]) and np.array_equal(out[:, 0], raw[:, 0, 0])


@pytest.mark.parametrize("how", ("nan_entry", "zero_over_zero"))
def test_a_bad_window_among_three(abn, oracle, gpu_ctx, hip, how):
    raw = _tables("plausible", 3, 40, seed=11)
    if how == "nan_entry":
        raw[1, 5, 2] = np.nan
        raw[1, 30, 6] = np.nan                               # a later one: the first is reported
    else:
        raw[1, 5, 0] = raw[1, 5, 1] = 0.0                    # alpha = beta = 0: beta / alpha is NaN, no entry is
    rc, _ = _host(abn, oracle, raw[1])
    assert rc == NO_FINITE_FIT
    with pytest.raises(abn.AbnError) as e:
        abn.analyze_batch(gpu_ctx, raw)
    assert e.value.status == NO_FINITE_FIT and "bootstrap 5" in str(e.value)
    out, fb = abn.analyze_batch(gpu_ctx, raw, allow_failed_windows=True)
    dout, dfb, again = _through_device_buffers(gpu_ctx, hip, raw, allow_failed_windows=True)
    for got, first_bad, name in ((out, fb, "abn_analyze_batch"), (dout, dfb, "abn_analyze_batch_dev")):
        assert first_bad.tolist() == [-1, 5, -1], name
        assert np.isnan(got[1]).all(), name
        for w in (0, 2):
            _assert_same(got[w], _host(abn, oracle, raw[w])[1], f"{name}, window {w}")
    assert np.isnan(again[1]).all() and not np.isnan(again[0]).any()
    with pytest.raises(abn.AbnError) as e:                    # the status of the device-resident entry
        _through_device_buffers(gpu_ctx, hip, raw)
    assert e.value.status == NO_FINITE_FIT


def test_argument_checks_with_a_context(abn, gpu_ctx):
    L = abn.load_library()
    raw, out, fb = _tables("plausible", 2, 8, seed=2), np.full((2, 32), -7.0), np.full(2, 9, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    praw, pout, pfb = raw.ctypes.data_as(dp), out.ctypes.data_as(dp), fb.ctypes.data_as(ip)
    h = gpu_ctx._h
    assert L.abn_analyze_batch(h, None, 2, 8, pout, pfb) == INVALID
    assert L.abn_analyze_batch(h, praw, 2, 8, None, pfb) == INVALID
    assert L.abn_analyze_batch(h, praw, -1, 8, pout, pfb) == INVALID
    assert L.abn_analyze_batch(h, praw, 2, 0, pout, pfb) == INVALID
    assert L.abn_analyze_batch(h, praw, 2, -8, pout, pfb) == INVALID
    assert L.abn_analyze_batch_dev(h, None, 2, 8, None, None, None) == INVALID
    assert L.abn_analyze_batch(h, praw, 0, 8, pout, pfb) == OK          # no windows: nothing is written
    assert np.all(out == -7.0) and np.all(fb == 9)
    assert L.abn_analyze_batch(h, praw, 2, 8, pout, None) == OK         # first_bad is optional
    assert not np.any(out == -7.0)


def _windows(golden, W):
    ped, p0 = golden["generated"], golden["p0uu_generated"]
    rng = np.random.default_rng(23)
    D = np.tile(ped[:, 3], (W, 1))
    D[1:] = np.abs(D[1:] * rng.uniform(0.7, 1.3, (W - 1, 1)))
    return ped, D, np.full(W, p0)


def test_plan_analyze(abn, oracle, gpu_ctx, hip, golden):
    """the bundled six-row pedigree, W = 3, S = 4, B = 41: Plan.analyze() is the host analysis of download()'s raw, from
    the plan's own table and from a caller's bound one"""
    W, S, B = 3, 4, 41
    ped, D, p0 = _windows(golden, W)
    plan = abn.Plan(gpu_ctx, ped[:, :3], W, S, B, options=abn.default_options(seed=9))
    bound = C.c_void_p()
    assert hip.hipMalloc(C.byref(bound), W * B * 7 * 8) == 0
    try:
        plan.set_windows(D, p0)
        with pytest.raises(abn.AbnError) as e:
            plan.analyze()
        assert e.value.status == STATE
        plan.run_phase(0)
        with pytest.raises(abn.AbnError) as e:                 # phase A alone leaves no table either
            plan.analyze()
        assert e.value.status == STATE
        plan.run_phase(1)
        out, fb = plan.analyze()
        raw = plan.download()["raw"]
        assert raw.shape == (W, B, 7) and np.all(fb == -1)
        for w in range(W):
            _assert_same(out[w], _host(abn, oracle, raw[w])[1], f"Plan.analyze, window {w}")
        # bound to a caller's buffer: the fits land there, and the analysis reads what that buffer holds
        plan.bind_raw(bound.value)
        plan.run()
        out2, fb2 = plan.analyze()
        raw2 = np.zeros((W, B, 7))
        assert hip.hipMemcpy(raw2.ctypes.data, bound, raw2.nbytes, 2) == 0
        assert np.array_equal(raw2, raw) and np.all(fb2 == -1)
        for w in range(W):
            _assert_same(out2[w], _host(abn, oracle, raw2[w])[1], f"Plan.analyze after bind_raw, window {w}")
        other = np.ascontiguousarray(raw[::-1] * 3.0)
        assert hip.hipMemcpy(bound, other.ctypes.data, other.nbytes, 1) == 0
        out3, _ = plan.analyze()
        for w in range(W):
            _assert_same(out3[w], _host(abn, oracle, other[w])[1], f"Plan.analyze of the bound buffer, window {w}")
        plan.bind_raw(0)                                       # back to the plan's own table, still the first run's
        out4, _ = plan.analyze()
        for w in range(W):
            _assert_same(out4[w], _host(abn, oracle, raw[w])[1], f"Plan.analyze after unbinding, window {w}")
    finally:
        plan.close()
        hip.hipFree(bound)


def test_multi_plan_analyze(abn, oracle, golden):
    W, S, B = 3, 4, 41
    ped, D, p0 = _windows(golden, W)
    mp = abn.MultiPlan([0], ped[:, :3], W, S, B, options=abn.default_options(seed=9))
    try:
        mp.set_windows(D, p0)
        with pytest.raises(abn.AbnError) as e:
            mp.analyze()
        assert e.value.status == STATE
        mp.run()
        out, fb = mp.analyze()
        raw = mp.download()["raw"]
        assert np.all(fb == -1)
        for w in range(W):
            _assert_same(out[w], _host(abn, oracle, raw[w])[1], f"MultiPlan.analyze, window {w}")
    finally:
        mp.close()
