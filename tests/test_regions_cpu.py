"""Region-level states (alphabeta_rs_amd/csrc/abn_regions.hpp) without a device: the serial form against the numpy model of
tests/_regions_model.py bit for bit; the walk of the kernel's lane and workgroup structure against the serial form on both
routes (windows walked by their lane, windows counted by the census first); the rule on planted counts; every refusal; the
stand-alone program of tests/native/regions_main.cpp plain and under the address and undefined-behaviour sanitizers; the
new symbols in the header, the prototype table and the documents; the compiled kernel's metadata; the CLI's flag errors."""
import itertools
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _regions_model as R
import _sim_model as S

ROOT = Path(__file__).resolve().parent.parent
CUTS = (0, 1, 15, 16, 17, 255, 256, 257)
RULES = ((1, 2, 3), (0, 1 << 10, 1 << 10), (5, 5, 9), (1 << 18, 3 << 18, 1 << 20))   # lo, hi, den; (0, den, den); lo = hi; den = 2^20
NEW_SYMBOLS = ("abn_packed_region_states", "abn_packed_region_states_dev", "abn_tiles_region_states", "abn_regions_destroy",
               "abn_regions_info", "abn_regions_layout", "abn_regions_order", "abn_regions_packed",
               "abn_regions_packed_device_ptr", "abn_regions_census", "abn_regions_pairwise", "abn_regions_transitions",
               "abn_regions_kernel_ms")


@pytest.fixture(scope="module")
def G():
    from alphabeta_rs_amd import regions

    return regions


def windows_of(L):
    """every pair of the cuts inside [0, L], an empty window, two overlapping windows, the whole row"""
    cuts = sorted({c for c in CUTS if c <= L} | {L})
    pairs = [(a, b) for a, b in itertools.combinations_with_replacement(cuts, 2)]
    pairs += [(L // 2, L // 2), (0, max(L - 1, 0)), (min(1, L), L), (0, L)]
    b, e = np.array(pairs, dtype=np.int64).T
    return b, e


def sources(rng, T):
    """identity; a permutation; repeats and omissions with C in 1, 15, 16, 17, 255, 256, 257"""
    yield None
    yield rng.permutation(T).astype(np.int32)
    for C in (1, 15, 16, 17, 255, 256, 257):
        yield rng.integers(0, T, size=C).astype(np.int32)


@pytest.fixture(scope="module")
def cases():
    """(packed, fields, L, begin, end) per (rows, L), made once"""
    rng = np.random.default_rng(20260101)
    out = []
    for rows in (1, 3):
        for L in (1, 15, 16, 17, 255, 256, 257, 4097):
            fields = R.random_fields(rng, rows, L)
            out.append((S.pack(fields), fields, L, *windows_of(L)))
    return out


def test_serial_form_equals_the_model(G, cases):
    rng = np.random.default_rng(7)
    seen_fields = set()
    for k, (packed, fields, L, b, e) in enumerate(cases):
        assert (fields == 3).any() or L < 255
        for j, src in enumerate(sources(rng, len(b))):
            lo, hi, den = RULES[(k + j) % len(RULES)]
            min_kept = (1, 2, 5)[(k + j) % 3]
            got = G.region_states_host(packed, L, b, e, lo, hi, den, min_kept, src=src)
            want = R.region_states(packed, L, b, e, (lo, hi, den, min_kept), src)
            assert got.dtype == np.uint8 and got.shape == want.shape and got.tobytes() == want.tobytes(), (L, j)
            C = len(b) if src is None else len(src)
            assert got.shape[1] == S.row_stride(C)
            unpacked = R.unpack(got, 4 * got.shape[1])
            assert (unpacked[:, C:] == 3).all()                                   # the padding up to the stride
            seen_fields |= set(np.unique(unpacked[:, :C]).tolist())
    assert seen_fields == {0, 1, 2, 3}


def test_every_rule_and_min_kept_on_one_matrix(G, cases):
    packed, fields, L, b, e = cases[-1]                                           # 3 rows of 4097 sites
    for (lo, hi, den), min_kept in itertools.product(RULES, (1, 2, 5)):
        got = G.region_states_host(packed, L, b, e, lo, hi, den, min_kept)
        assert got.tobytes() == R.region_states(packed, L, b, e, (lo, hi, den, min_kept)).tobytes()


def test_walk_equals_the_serial_form_on_both_routes(G, cases):
    """long_sites 0 (the default) and 64 (windows of 63 sites are walked by their
    lane, of 64 and 65 counted by the census's walk)"""
    rng = np.random.default_rng(11)
    for k, (packed, fields, L, b, e) in enumerate(cases):
        if L >= 257:                                                              # windows of 63, 64 and 65 sites, off the dword grid
            b = np.concatenate((b, [3, 3, 3, 100, 101, 102])).astype(np.int64)
            e = np.concatenate((e, [66, 67, 68, 163, 165, 167])).astype(np.int64)
            assert {63, 64, 65} <= set((e - b).tolist())
        for j, src in enumerate(sources(rng, len(b))):
            lo, hi, den = RULES[(k + j) % len(RULES)]
            serial = G.region_states_host(packed, L, b, e, lo, hi, den, 1 + j % 2, src=src)
            for long_sites in (0, 64):
                walk = G.region_states_host(packed, L, b, e, lo, hi, den, 1 + j % 2, src=src, long_sites=long_sites, walk=True)
                assert walk.tobytes() == serial.tobytes(), (L, j, long_sites)
    source = (ROOT / "alphabeta_rs_amd" / "csrc" / "abn_regions.hpp").read_text()
    default = int(re.search(r"constexpr long long kRegionLongSites = (\d+);", source).group(1))
    assert default > 64 and default % 256 == 0


def test_call_on_planted_counts(G):
    lo, hi, den = 1, 2, 3                                 # thresholds: 3 m = 2 kept and 3 m = 4 kept
    assert G.call_host(1, 2, 0, lo, hi, den) == 1         # kept 3, m 2: equality below
    assert G.call_host(0, 2, 1, lo, hi, den) == 1         # kept 3, m 4: equality above
    assert G.call_host(2, 1, 0, lo, hi, den) == 0 and G.call_host(0, 1, 2, lo, hi, den) == 2      # one unit on either side
    assert G.call_host(4, 2, 0, lo, hi, den, 7) == 3 and G.call_host(4, 2, 1, lo, hi, den, 7) == R.call(4, 2, 1, lo, hi, den, 7) != 3
    assert G.call_host(0, 0, 0, 0, 4, 4) == 3             # an empty window
    big, den = 1 << 34, 1 << 20
    for n0, n1, n2 in ((big, 0, 0), (0, big, 0), (0, 0, big), (big // 2, 0, big // 2), (big // 2, 1, big // 2 - 1),
                       (big // 2 - 1, 1, big // 2), (big - 3, 2, 1)):
        for lo, hi in ((den // 2, den // 2), (0, den), (1, den - 1), (den, den), (0, 0)):
            assert G.call_host(n0, n1, n2, lo, hi, den) == R.call(n0, n1, n2, lo, hi, den), (n0, n1, n2, lo, hi)
    assert G.call_host(big // 2, 0, big // 2, den // 2, den // 2, den) == 1
    assert G.call_host(big // 2, 1, big // 2 - 1, den // 2, den // 2, den) == 0
    rng = np.random.default_rng(3)
    for _ in range(2000):
        n0, n1, n2 = (int(x) for x in rng.integers(0, 40, size=3))
        d = int(rng.integers(1, 50))
        lo = int(rng.integers(0, d + 1))
        hi = int(rng.integers(lo, d + 1))
        mk = int(rng.integers(1, 6))
        assert G.call_host(n0, n1, n2, lo, hi, d, mk) == R.call(n0, n1, n2, lo, hi, d, mk)


def test_refusals(G, abn):
    rng = np.random.default_rng(5)
    packed = S.pack(R.random_fields(rng, 2, 300))
    b, e = np.array([0, 10], dtype=np.int64), np.array([5, 300], dtype=np.int64)

    def refused(word, *, packed=packed, n_sites=300, b=b, e=e, rule=(1, 2, 3, 1), **kw):
        with pytest.raises(abn.AbnError) as err:
            G.region_states_host(packed, n_sites, b, e, *rule, **kw)
        assert err.value.status == 1 and word in str(err.value), str(err.value)

    assert G.region_states_host(packed, 300, b, e, 1, 2, 3, 1).shape == (2, 64)
    assert G.region_states_host(packed, 300, b, e, 1, 2, 3, 1, src=np.zeros(0, dtype=np.int32)).shape == (2, 0)   # C = 0: no error
    # the census's: the stride, the samples, the windows
    refused("row_stride_bytes", packed=packed[:, :32])
    refused("row_stride_bytes", n_sites=600)
    refused("window 1", e=np.array([5, 301], dtype=np.int64))
    refused("window 0", b=np.array([6, 10], dtype=np.int64))
    refused("null/size", n_sites=-1)
    # the rule
    for rule in ((2, 1, 3, 1), (1, 4, 3, 1), (-1, 2, 3, 1), (1, 2, 0, 1), (1, 2, (1 << 20) + 1, 1)):
        refused("lo_num <= hi_num <= den", rule=rule)
    refused("min_kept", rule=(1, 2, 3, 0))
    # the column map
    refused("column 1", src=np.array([0, 2, 1], dtype=np.int32))
    refused("column 0", src=np.array([-1], dtype=np.int32))
    refused("n_columns is not n_windows", n_columns=3)
    # the counts
    refused("INT32_MAX", src=np.zeros(1, dtype=np.int32), n_columns=1 << 31)
    # long_sites
    refused("long_sites", long_sites=-16)
    refused("long_sites", long_sites=40)
    with pytest.raises(abn.AbnError):
        G.call_host(1, 1, 1, 2, 1, 3)


def build_native(tmp_path, name, *flags):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed for tests/native/regions_main.cpp")
    exe = tmp_path / name
    r = subprocess.run([gxx, "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, "-o", str(exe),
                        str(ROOT / "tests" / "native" / "regions_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_native_program_plain(tmp_path):
    r = subprocess.run([str(build_native(tmp_path, "regions_main", "-O2"))], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "regions ok" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_native_program_under_address_and_ub_sanitizers(tmp_path):
    """A stand-alone program (its own main, run directly): the walk against the serial form, every array in a heap block of
    exactly its length, built with -fsanitize=address,undefined."""
    exe = build_native(tmp_path, "regions_main_san", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"})
    assert r.returncode == 0 and "regions ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_new_symbols_are_declared_bound_and_documented():
    from alphabeta_rs_amd import _ffi

    header = (ROOT / "include" / "abneutral.h").read_text()
    docs = {name: (ROOT / name).read_text() for name in ("README.md", "DESIGN.md", "INTEGRATION.md")}
    for sym in NEW_SYMBOLS:
        assert re.search(rf"\bint {sym}\(", header), sym
        assert sym in _ffi.PROTOTYPES, sym
        for name, text in docs.items():
            assert sym in text, (sym, name)
    assert "typedef struct abn_regions abn_regions;" in header
    assert "abn_regions.hip" in (ROOT / "alphabeta_rs_amd" / "build.py").read_text()
    for host_only in ("abn_packed_region_states_host", "abn_region_call_host"):    # the host library's, not the header's
        assert host_only not in header


def test_kernel_metadata_declares_no_lds_and_no_private_segment():
    from _device_isa import CSRC, device_isa
    from test_sim_study_isa import _kernels, _sizes

    kernels = _kernels(device_isa(src=CSRC / "abn_regions.hip"), "abn_region_states_kernel")
    assert len(kernels) == 1, sorted(kernels)
    for name, desc in kernels.items():
        assert _sizes(desc, name) == (0, 0), name


# ---- the CLI's refusals that happen before the device is opened
def run_cli(*args):
    from alphabeta_rs_amd import build as B

    B.build_host()
    return subprocess.run([str(B.META_CLI), *map(str, args)], capture_output=True, text=True, timeout=120)


def test_cli_flag_errors(tmp_path):
    (tmp_path / "regions.bed").write_text("1\t0\t100\tgene\n")
    base = ["-o", tmp_path, "--methylome", tmp_path, "--nodes", tmp_path / "n", "--edges", tmp_path / "e"]
    tiled = [*base, "--tiles", "1000"]

    def refused(word, *args):
        r = run_cli(*args)
        assert r.returncode == 2 and word in r.stderr, (args, r.stdout[-500:], r.stderr[-500:])

    refused("--region-states belongs to --tiles and --regions", "-o", tmp_path, "--region-states", "0.25,0.75")
    refused("--region-states belongs to --tiles and --regions", *base, "--genome", tmp_path / "g", "--region-states", "0.25,0.75")
    refused("--region-min-sites belongs to --region-states", *tiled, "--region-min-sites", "2")
    refused("block", *tiled, "--region-states", "0.25,0.75", "--block-bootstrap", "10")
    for bad in ("0.25", "0.25,", ",0.75", "0.75,0.25", "0.25,1.5", "-0.1,0.5", "0.25;0.75", "0.1234567,0.5", "a,b", "0.25,0.75,1",
                "1e-1,0.5", " 0.25,0.75", "0.25,0.75 ", "1.0000001,1", ".,1", ""):
        refused("--region-states expects", *tiled, "--region-states", bad)
    for bad in ("0", "-1", "x", "1.5", "", " 3", "+3", "3 ", "0x3"):
        refused("--region-min-sites expects", *tiled, "--region-states", "0.25,0.75", "--region-min-sites", bad)
    # what is accepted gets past the flags: the run then fails on the files that do not exist, not on a flag (exit 1)
    for good in ("0.25,0.75", "0,1", "1,1", "0.000001,1.000000", ".5,.5", "0.,1."):
        r = run_cli(*tiled, "--region-states", good, "--region-min-sites", "3")
        assert r.returncode == 1 and "expects" not in r.stderr, (good, r.stdout[-500:], r.stderr[-500:])
