"""The window edges of the packed windows scan (csrc/abn_packed_mask.hpp; DMatrix::from, src/pedigree.rs:210-261, in the
window loop of src/cli/metaprofile.rs:50-72) on the CPU: the mask that makes the sites outside a column range read as
filtered, as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer — nothing is loaded into python."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "alphabeta_rs_amd" / "csrc"

_MAIN = r"""
// abn_packed_outside_mask / abn_packed_window_mask against abn_unpack_codes: a dword of sixteen random fields, every
// (lo, hi) with 0 <= lo <= hi <= 16 — the sites inside are unchanged, the sites outside are filtered
#include <cstdio>
#include <cstring>
#include <vector>
#include "abneutral.h"
#include "abn_packed_mask.hpp"

static unsigned long long state = 88172645463325252ull;
static unsigned rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (unsigned)(state >> 11); }
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// the sixteen sites of dword g of a one-row packed matrix of exactly `bytes` bytes
static int unpack16(const std::vector<unsigned char>& row, int g, unsigned char* out) {
  std::vector<unsigned char> codes(row.size() * 4);
  if (abn_unpack_codes(row.data(), 1, (long long)codes.size(), (long long)row.size(), codes.data(),
                       (long long)codes.size()) != ABN_OK)
    return 1;
  std::memcpy(out, codes.data() + 16 * g, 16);
  return 0;
}

int main() {
  static_assert(abn::kPmxWinPackedChunkSites % 256 == 0 && abn::kPmxWinPackedChunkSites < (1ll << 30), "chunk");
  int cases = 0;
  for (int lo = 0; lo <= 16; ++lo)
    for (int hi = lo; hi <= 16; ++hi)
      for (int rep = 0; rep < 24; ++rep) {
        const int g = rep % 16;                      // which dword of the 64-byte row
        std::vector<unsigned char> row(64), masked(64);
        for (auto& b : row) b = (unsigned char)rnd();
        if (rep == 0) std::memset(row.data(), 0x00, 64);   // all U: every forced bit shows
        if (rep == 1) std::memset(row.data(), 0xaa, 64);   // all M
        masked = row;
        uint32_t w;
        std::memcpy(&w, row.data() + 4 * g, 4);      // little-endian, as the device reads it
        const uint32_t m = abn::abn_packed_outside_mask(lo, hi);
        w |= m;
        std::memcpy(masked.data() + 4 * g, &w, 4);
        unsigned char before[16], after[16];
        CHECK(unpack16(row, g, before) == 0 && unpack16(masked, g, after) == 0);
        for (int s = 0; s < 16; ++s) {
          if (s >= lo && s < hi) CHECK(after[s] == before[s]);
          else CHECK(after[s] == 0x80);
        }
        // the same mask from a column range of the row, wherever the range begins and ends outside the dword
        const int site0 = 16 * g;
        CHECK(abn::abn_packed_window_mask(site0, site0 + lo, site0 + hi) == (lo < hi ? m : 0xffffffffu));
        if (lo == 0) CHECK(abn::abn_packed_window_mask(site0, site0 - 1 - (int)(rnd() % 300), site0 + hi) == (hi ? m : 0xffffffffu));
        if (hi == 16) CHECK(abn::abn_packed_window_mask(site0, site0 + lo, site0 + 16 + (int)(rnd() % 300)) == (lo < 16 ? m : 0xffffffffu));
        ++cases;
      }
  // a range that misses the dword on either side filters all of it; one that covers it changes nothing
  CHECK(abn::abn_packed_window_mask(32, 0, 32) == 0xffffffffu && abn::abn_packed_window_mask(32, 48, 256) == 0xffffffffu);
  CHECK(abn::abn_packed_window_mask(32, 0, 256) == 0u && abn::abn_packed_window_mask(32, 32, 48) == 0u);
  CHECK(abn::abn_packed_outside_mask(0, 16) == 0u && abn::abn_packed_outside_mask(7, 7) == 0xffffffffu);
  // pinned by hand: keep sites 5..6 = byte 1 and byte 2 of shift j = 1 (bits 2..3)
  CHECK(abn::abn_packed_outside_mask(5, 7) == (0xffffffffu & ~(0x0cu << 8) & ~(0x0cu << 16)));
  std::printf("sanitized masks ok %d\n", cases);
  return 0;
}
"""


def test_window_mask_under_address_and_ub_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is a requirement of the CPU tier (the oracle and this program are built with it)"
    main = tmp_path / "mask_main.cpp"
    main.write_text(_MAIN)
    exe = tmp_path / "mask_asan"
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", str(ROOT / "include"), "-I", str(CSRC),
                        "-o", str(exe), str(main), str(CSRC / "abn_pack.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sanitized masks ok %d" % (153 * 24) in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_binding_lists_the_packed_windows_entries(abn):
    """no device needed: the symbols are exported and bound"""
    L = abn.load_library(build_if_missing=True)
    for name in ("abn_pairwise_divergence_windows_packed", "abn_pairwise_divergence_windows_packed_dev"):
        assert name in abn.EXPORTED_SYMBOLS and getattr(L, name).argtypes is not None
    assert hasattr(abn.Context, "pairwise_divergence_windows_packed")
    assert hasattr(abn.Context, "pairwise_divergence_windows_packed_dev")


# ---- the layout of Pedigree::build_many's scan calls (host/pedigree_build.hpp: PackedBatch, layout_packed_call) through
# its shim in host/host_capi.cpp, on the window directories of tests/_build_many.py: no device

def _layout(H, lists, cap_bytes, flt=0.99):
    import ctypes as C

    import numpy as np

    W = len(lists)
    nls = (C.c_char_p * W)(*[a.encode() for a, _ in lists])
    els = (C.c_char_p * W)(*[b.encode() for _, b in lists])
    call_of, n_samples = np.zeros(W, dtype=np.int32), np.zeros(W, dtype=np.int32)
    n_sites, begin, end, codes_off = (np.zeros(W, dtype=np.int64) for _ in range(4))
    stride, packed_off = np.zeros(W, dtype=np.int64), np.zeros(W, dtype=np.int64)
    codes_out, packed_out = np.full(1 << 16, 0x55, dtype=np.uint8), np.full(1 << 16, 0x55, dtype=np.uint8)
    i32p, i64p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    H.abh_build_many_layout.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int, C.c_double, C.c_longlong,
                                        i32p, i32p, i64p, i64p, i64p, i64p, u8p, C.c_longlong, i64p, i64p, u8p,
                                        C.c_longlong]
    ncalls = H.abh_build_many_layout(nls, els, W, flt, cap_bytes, call_of.ctypes.data_as(i32p),
                                     n_samples.ctypes.data_as(i32p), n_sites.ctypes.data_as(i64p),
                                     begin.ctypes.data_as(i64p), end.ctypes.data_as(i64p), codes_off.ctypes.data_as(i64p),
                                     codes_out.ctypes.data_as(u8p), codes_out.size, stride.ctypes.data_as(i64p),
                                     packed_off.ctypes.data_as(i64p), packed_out.ctypes.data_as(u8p), packed_out.size)
    assert ncalls >= 0
    entries = []
    for w in range(W):
        codes = None
        if call_of[w] >= 0:
            codes = codes_out[codes_off[w]: codes_off[w] + n_samples[w] * n_sites[w]].reshape(n_samples[w], n_sites[w])
        entries.append({"call": int(call_of[w]), "samples": int(n_samples[w]), "sites": int(n_sites[w]),
                        "begin": int(begin[w]), "end": int(end[w]), "codes": codes})
    nn = max(e["samples"] for e in entries if e["call"] >= 0)
    calls = [packed_out[packed_off[k]: packed_off[k] + nn * stride[k]].reshape(nn, stride[k]) for k in range(ncalls)]
    return entries, calls


def _check_calls(abn, entries, calls):
    """every entry's columns unpack to its write_codes bytes; every other field of its call's matrix is 3"""
    import numpy as np

    for k, packed in enumerate(calls):
        nn, stride = packed.shape
        assert stride % 64 == 0 and stride >= 64
        unpacked = abn.unpack_codes(packed, 4 * stride)           # 0x80: the field is 3
        covered = np.zeros(4 * stride, dtype=bool)
        last_end = 0
        for e in (e for e in entries if e["call"] == k):
            assert e["samples"] == nn
            assert e["begin"] % 256 == 0 and e["end"] - e["begin"] == e["sites"]
            assert e["begin"] >= last_end and e["end"] <= 4 * stride       # in order, no overlap
            last_end = e["end"]
            want = np.where(e["codes"] & 0x80, 0x80, e["codes"]).astype(np.uint8)
            assert set(np.unique(want)) <= {0, 1, 2, 0x80}
            assert np.array_equal(unpacked[:, e["begin"]: e["end"]], want)
            covered[e["begin"]: e["end"]] = True
        assert covered.any() and not covered.all()                          # there are gap / padding fields
        assert np.all(unpacked[:, ~covered] == 0x80)


def test_build_many_layout_of_one_call(abn, tmp_path):
    from _build_many import hostlib, write_windows

    golden = Path(__file__).resolve().parent / "golden"
    H = hostlib()
    lists = write_windows(tmp_path, golden)
    entries, calls = _layout(H, lists, 1 << 30)
    # window 2 has no nodelist, window 3 another sample count, window 5 samples of unequal length: not in this scan
    assert [e["call"] for e in entries] == [0, 0, -1, -1, 0, -1, 0]
    assert entries[2]["samples"] == -1 and entries[3]["samples"] == 3 and entries[5]["samples"] == 4
    scan = [e for e in entries if e["call"] == 0]
    assert [e["sites"] for e in scan] == [120, 150, 240, 300]
    assert [e["begin"] for e in scan] == [0, 256, 512, 768] and calls[0].shape == (4, 320)
    assert any((e["codes"] & 0x80).any() for e in scan) and any((e["codes"] == 2).any() for e in scan)
    assert len(calls) == 1
    _check_calls(abn, entries, calls)


def test_build_many_layout_a_low_byte_cap_cuts_the_group_in_order(abn, tmp_path):
    from _build_many import hostlib, write_windows

    golden = Path(__file__).resolve().parent / "golden"
    H = hostlib()
    lists = [p for k, p in enumerate(write_windows(tmp_path, golden)) if k in (0, 1, 4, 6)]
    # four samples; the entries take 64, 64, 64 and 128 bytes of a row: 512 bytes hold the first two, then one each
    entries, calls = _layout(H, lists, 4 * 128)
    assert [e["call"] for e in entries] == [0, 0, 1, 2]
    assert [c.shape for c in calls] == [(4, 128), (4, 64), (4, 128)]
    assert [e["begin"] for e in entries] == [0, 256, 0, 0]
    _check_calls(abn, entries, calls)
    # a cap below any entry still takes one entry per call
    entries, calls = _layout(H, lists, 1)
    assert [e["call"] for e in entries] == [0, 1, 2, 3]
    _check_calls(abn, entries, calls)
