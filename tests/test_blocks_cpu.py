"""The block bootstrap (abn_block_*, alphabeta_rs_amd/csrc/abn_blocks.hpp) without a device: the serial host forms
abn_block_resample_host and abn_block_counts_host against the model of tests/_blocks_model.py bit for bit, the header's
constants against their derivations, and every refusal of the host-only argument check."""
import ctypes as C

import numpy as np
import pytest

import _blocks_model as M

NEW_SYMBOLS = ["abn_block_counts", "abn_block_counts_host", "abn_block_resample", "abn_block_resample_dev",
               "abn_block_resample_host", "abn_tiles_block_bootstrap", "abn_tiles_block_groups", "abn_tiles_block_ms"]
K = M.constants()


@pytest.mark.parametrize("case", M.product_cases(), ids=lambda c: c[0])
def test_resample_host_equals_the_model(abn, case):
    gb, ge, counts, both, diff, lsk, kept = M.product_inputs(case)
    got = abn.block_resample_host(gb, ge, counts, both, diff, lsk, kept)
    M.assert_equal(got, M.resample(gb, ge, counts, both, diff, lsk, kept))
    if case[0] == "three-groups":
        assert not got["both"][1].any() and np.isnan(got["dvalue"][1]).all() and not got["level"][1].any()   # the empty group
        assert {0, 1, 127} <= set(np.unique(counts).tolist()) and int(both.max()) == (1 << 35) - 1


def test_resample_host_flush_case(abn):
    args = M.flush_inputs(K["kBlockFlush"])
    got = abn.block_resample_host(*args)
    T = K["kBlockFlush"] + 65
    assert int(got["both"][0, 0, 0]) == 127 * ((1 << 35) - 1) * T
    M.assert_equal(got, M.resample(*args))


def test_constants_and_their_derivations():
    assert 127 * 127 * K["kBlockFlush"] < 1 << 31 and K["kBlockFlush"] % 64 == 0
    assert 127 * 127 * 2 * K["kBlockFlush"] >= 1 << 31                           # the next power of two would overflow
    assert K["kBlockCountMax"] == 127 and K["kBlockDigitBits"] == 7
    assert K["kBlockCountMax"] * K["kBlockValueEnd"] * K["kBlockGroupMax"] <= 1 << 63
    assert K["kBlockValueEnd"] == 1 << 35 and K["kBlockGroupMax"] == 1 << 21
    assert K["kBlockDigitsMax"] == -(-35 // 7)
    assert K["kBlockReplicatesMax"] == (1 << 20) - 2 and K["kBlockGroupsMax"] == 4096
    assert 4 * K["kBlockHist"] <= 64 * 1024 and K["kBlockHist"] > 257            # 32-bit bins in a workgroup's static LDS


def test_counts_host_equal_the_model(abn, oracle):
    sizes = M.count_group_sizes(K["kBlockHist"])
    gb = np.concatenate([[2], 2 + np.cumsum(sizes)[:-1] + np.arange(1, len(sizes))]).astype(np.int64)   # a gap between groups
    ge = gb + np.array(sizes)
    gid = np.array([7, 0, 3, 4095, 11, 12, 13, 2 ** 32 - 1], dtype=np.uint32)
    T = int(ge[-1]) + 3
    got = abn.block_counts_host(20260101, gid, gb, ge, 2, T)
    want = M.counts(oracle, 20260101, gid, gb, ge, 2, T)
    assert got.dtype == np.uint8 and got.shape == want.shape and got.tobytes() == want.tobytes()
    for g, size in enumerate(sizes):
        assert got[g].sum(axis=1).tolist() == [size] * 3                         # every row makes T_g draws
        assert got[g, 2, gb[g]:ge[g]].tolist() == [1] * size and got[g, :, :gb[g]].sum() == 0 == got[g, :, ge[g]:].sum()
    # a row depends on neither R nor G
    fewer = abn.block_counts_host(20260101, gid[3:5], gb[3:5], ge[3:5], 1, T)
    assert fewer[:, 0].tobytes() == got[3:5, 0].tobytes() and fewer[:, 1].tobytes() == got[3:5, 2].tobytes()
    assert abn.block_counts_host(20260102, gid[3:5], gb[3:5], ge[3:5], 1, T)[:, 0].tobytes() != fewer[:, 0].tobytes()


def refused(abn, call, *args, words):
    with pytest.raises(abn.AbnError) as e:
        call(*args)
    assert e.value.status == M.INVALID and words in str(e.value), str(e.value)


def test_every_refusal_comes_from_the_host_check(abn):
    gb, ge, counts, both, diff, lsk, kept = M.product_inputs(M.product_cases()[0])
    ok = (gb, ge, counts, both, diff, lsk, kept)
    abn.block_resample_host(*ok)

    def with_(**kw):
        names = ("gb", "ge", "counts", "both", "diff", "lsk", "kept")
        return tuple(kw.get(k, v) for k, v in zip(names, ok))

    big = both.copy()
    big[0, 0] = 1 << 35
    refused(abn, abn.block_resample_host, *with_(both=big), words="2^35")
    refused(abn, abn.block_resample_host, *with_(diff=big), words="2^35")
    over = counts.copy()
    over[0, 0, 3] = 128
    refused(abn, abn.block_resample_host, *with_(counts=over), words="above 127")
    outside = counts.copy()
    outside[0, 0, 0] = 255                                                       # outside the group's range: never read
    abn.block_resample_host(*with_(counts=outside))
    # the groups
    T = counts.shape[2]
    refused(abn, abn.block_resample_host, *with_(gb=np.array([5]), ge=np.array([4])), words="unordered")
    refused(abn, abn.block_resample_host, *with_(ge=np.array([T + 1])), words="unordered")
    two = np.zeros((2,) + counts.shape[1:], dtype=np.uint8)
    refused(abn, abn.block_resample_host, np.array([0, 2]), np.array([3, 4]), two, both, diff, lsk, kept, words="overlaps")
    refused(abn, abn.block_resample_host, np.array([3, 0]), np.array([4, 2]), two, both, diff, lsk, kept, words="unordered")
    many = K["kBlockGroupsMax"] + 1
    empty = (np.zeros((0, 1), dtype=np.uint64), np.zeros((0, 1), dtype=np.uint64), np.zeros((1, 0)), np.zeros((1, 0), dtype=np.int64))
    refused(abn, abn.block_resample_host, np.zeros(many), np.zeros(many), np.zeros((many, 1, 0), dtype=np.uint8), *empty,
            words="4096 groups")
    abn.block_resample_host(np.zeros(many - 1), np.zeros(many - 1), np.zeros((many - 1, 1, 0), dtype=np.uint8), *empty)
    rows = K["kBlockReplicatesMax"] + 2
    refused(abn, abn.block_resample_host, [0], [0], np.zeros((1, rows, 0), dtype=np.uint8), *empty, words="replicates")
    abn.block_resample_host([0], [0], np.zeros((1, rows - 1, 0), dtype=np.uint8), *empty)
    refused(abn, abn.block_counts_host, 1, [0], [0], [0], K["kBlockReplicatesMax"] + 1, 0, words="replicates")
    refused(abn, abn.block_counts_host, 1, [0], [0], [0], -1, 0, words="negative")
    long = K["kBlockGroupMax"] + 1
    none = (np.zeros((long, 0), dtype=np.uint64), np.zeros((long, 0), dtype=np.uint64), np.zeros((0, long)),
            np.zeros((0, long), dtype=np.int64))
    refused(abn, abn.block_resample_host, [0], [long], np.zeros((1, 1, long), dtype=np.uint8), *none, words="2^21 blocks")
    abn.block_resample_host([1], [long], np.zeros((1, 1, long), dtype=np.uint8), *none)
    # null pointers and negative sizes: the C entry itself
    L = abn.load_library()
    text = C.create_string_buffer(256)
    i64p = C.POINTER(C.c_int64)
    g = (gb.ctypes.data_as(i64p), ge.ctypes.data_as(i64p))
    assert L.abn_block_resample_host(1, None, None, 1, None, T, 0, 0, *[None] * 9, text, 256) == M.INVALID and b"null" in text.value
    assert L.abn_block_resample_host(1, *g, 1, None, T, 0, 0, *[None] * 9, text, 256) == M.INVALID and b"null" in text.value
    cp = counts.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.abn_block_resample_host(1, *g, 1, cp, T, 1, 0, *[None] * 9, text, 256) == M.INVALID and b"null" in text.value
    assert L.abn_block_resample_host(1, *g, 1, cp, T, 0, 1, *[None] * 9, text, 256) == M.INVALID and b"null" in text.value
    for sizes in ((-1, *g, 1, cp, T, 0, 0), (1, *g, -1, cp, T, 0, 0), (1, *g, 1, cp, -1, 0, 0), (1, *g, 1, cp, T, -1, 0),
                  (1, *g, 1, cp, T, 0, -1)):
        assert L.abn_block_resample_host(*sizes, *[None] * 9, text, 256) == M.INVALID and b"negative" in text.value, sizes
    assert L.abn_block_resample_host(1, *g, 1, cp, T, 0, 0, *[None] * 9, None, 0) == 0          # nothing to sum: no error
    assert L.abn_block_counts_host(1, 1, None, *g, 1, T, None, text, 256) == M.INVALID and b"null" in text.value
    assert L.abn_block_counts(None, 1, 1, None, *g, 1, T, None) == M.INVALID


def test_new_symbols_are_exported_and_documented(abn):
    from pathlib import Path

    root = Path(abn.__file__).resolve().parent.parent
    L = abn.load_library()
    doc, header = (root / "INTEGRATION.md").read_text(), (root / "include" / "abneutral.h").read_text()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in abn.EXPORTED_SYMBOLS and f"{name}(" in doc and f"{name}(" in header


@pytest.mark.parametrize("sanitize", [False, True])
def test_standalone_driver(tmp_path, sanitize):
    """tests/native/blocks_main.cpp, a program of its own (nothing is loaded into Python): plain, and with
    -fsanitize=address,undefined, every array in a heap block of exactly its length"""
    import shutil
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed for tests/native/blocks_main.cpp")
    exe = tmp_path / "blocks_main"
    flags = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else []
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", *flags, "-o", str(exe),
                        str(root / "tests" / "native" / "blocks_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                       env={"UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1", "ASAN_OPTIONS": "abort_on_error=1"})
    assert r.returncode == 0 and "block bootstrap serial forms ok" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
