"""The 2-bit packed code format of the pairwise scan (include/abneutral.h: abn_packed_row_stride, abn_pack_codes,
abn_unpack_codes; DMatrix::from, src/pedigree.rs:210-261) — host arithmetic through ctypes, no device: the layout pinned
by hand, the row stride, round trips against a numpy model of the layout, the refusals, and the pack / unpack translation
unit (csrc/abn_pack.cpp) as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
U8P = C.POINTER(C.c_uint8)
INVALID = 1  # ABN_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def lib(abn):
    L = abn.load_library(build_if_missing=True)
    for name in ("abn_packed_row_stride", "abn_pack_codes", "abn_unpack_codes"):
        getattr(L, name)                       # AttributeError: the library lacks the packed format
    return L


def _p(a):
    return a.ctypes.data_as(U8P)


def model_pack(codes, stride):
    """numpy model of the layout: site 16 g + 4 j + e -> byte 4 g + e of the row, bits 2j..2j+1; padding fields 3"""
    n, L = codes.shape
    field = np.where(codes & 0x80, 3, codes & 3).astype(np.uint8)
    full = np.full((n, stride * 4), 3, dtype=np.uint8)      # one field per site the row has room for
    full[:, :L] = field
    g = full.reshape(n, stride // 4, 4, 4)                  # [row][dword g][j][e]
    out = np.zeros((n, stride // 4, 4), dtype=np.uint8)     # [row][dword g][byte e]
    for j in range(4):
        out |= g[:, :, j, :] << (2 * j)
    return out.reshape(n, stride)


def canonical(codes):
    return np.where(codes & 0x80, 0x80, codes).astype(np.uint8)


def random_codes(rng, n, L, src_stride):
    buf = rng.integers(0, 256, size=(n, src_stride), dtype=np.uint8)   # junk behind the sites: never read as codes
    status = rng.integers(0, 3, size=(n, L), dtype=np.uint8)
    flag = np.where(rng.random((n, L)) < 0.3, 0x80 | (rng.integers(0, 128, size=(n, L)) & 0x7f), 0).astype(np.uint8)
    buf[:, :L] = np.where(flag, flag, status)
    return buf


def test_layout_pinned_by_hand(lib):
    codes = np.array([[k % 3 for k in range(16)]], dtype=np.uint8)
    codes[0, 5] |= 0x80
    codes[0, 14] = 0x80
    want = 0
    for k in range(16):
        f = 3 if k in (5, 14) else k % 3
        j, e = (k % 16) // 4, k % 4
        want |= f << (8 * e + 2 * j)
    packed = np.zeros((1, 64), dtype=np.uint8)
    assert lib.abn_pack_codes(_p(codes), 1, 16, 16, _p(packed), 64) == 0
    assert int.from_bytes(packed[0, :4].tobytes(), "little") == want
    assert np.all(packed[0, 4:] == 0xFF)
    for j in range(4):                                     # the kernel's view: four byte-sized codes per shift
        quad = (want >> (2 * j)) & 0x03030303
        assert [(quad >> (8 * e)) & 0xFF for e in range(4)] == [3 if 4 * j + e in (5, 14) else (4 * j + e) % 3
                                                                 for e in range(4)]


def test_packed_row_stride(lib, abn):
    for L, want in ((0, 0), (1, 64), (256, 64), (257, 128)):
        assert lib.abn_packed_row_stride(L) == want
        assert abn.packed_row_stride(L) == want


@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("L", [0, 1, 15, 16, 17, 255, 256, 257, 1000])
def test_round_trip_and_model(lib, n, L):
    rng = np.random.default_rng(1000 * n + L)
    src_stride = L + 13
    codes = random_codes(rng, n, L, src_stride)
    for stride in (lib.abn_packed_row_stride(L), lib.abn_packed_row_stride(L) + 128):
        packed = np.zeros((n, stride), dtype=np.uint8)
        assert lib.abn_pack_codes(_p(codes), n, L, src_stride, _p(packed), stride) == 0
        assert np.array_equal(packed, model_pack(codes[:, :L], stride))
        back = np.full((n, src_stride), 0x55, dtype=np.uint8)
        assert lib.abn_unpack_codes(_p(packed), n, L, stride, _p(back), src_stride) == 0
        assert np.array_equal(back[:, :L], canonical(codes[:, :L]))
        assert np.all(back[:, L:] == 0x55)                 # nothing behind the sites is written


def test_python_wrappers_round_trip(abn):
    rng = np.random.default_rng(5)
    codes = random_codes(rng, 5, 300, 300)
    packed = abn.pack_codes(codes)
    assert packed.shape == (5, 128) and np.array_equal(packed, model_pack(codes, 128))
    assert np.array_equal(abn.unpack_codes(packed, 300), canonical(codes))
    assert abn.pack_codes(codes, row_stride=256).shape == (5, 256)
    with pytest.raises(abn.AbnError):
        abn.pack_codes(np.full((1, 4), 3, dtype=np.uint8))


def test_refusals(lib):
    ok = np.zeros((2, 20), dtype=np.uint8)
    out = np.zeros((2, 128), dtype=np.uint8)
    assert lib.abn_pack_codes(_p(ok), 2, 20, 20, _p(out), 64) == 0
    for bad in (3, 0x40):
        codes = ok.copy()
        codes[1, 7] = bad
        assert lib.abn_pack_codes(_p(codes), 2, 20, 20, _p(out), 64) == INVALID
    assert lib.abn_pack_codes(_p(ok), 2, 20, 20, _p(out), 32) == INVALID          # not a multiple of 64
    assert lib.abn_pack_codes(_p(ok), 2, 20, 20, _p(out), 96) == INVALID
    long = np.zeros((1, 257), dtype=np.uint8)
    assert lib.abn_pack_codes(_p(long), 1, 257, 257, _p(out), 64) == INVALID      # below the minimum (128)
    assert lib.abn_pack_codes(_p(long), 1, 257, 257, _p(out), 128) == 0
    assert lib.abn_pack_codes(_p(ok), 2, 20, 19, _p(out), 64) == INVALID          # source rows shorter than n_sites
    assert lib.abn_pack_codes(None, 2, 20, 20, _p(out), 64) == INVALID
    assert lib.abn_pack_codes(_p(ok), 2, 20, 20, None, 64) == INVALID
    assert lib.abn_unpack_codes(None, 2, 20, 64, _p(ok), 20) == INVALID
    assert lib.abn_unpack_codes(_p(out), 2, 20, 64, None, 20) == INVALID
    assert lib.abn_unpack_codes(_p(out), 2, 20, 32, _p(ok), 20) == INVALID
    assert lib.abn_unpack_codes(_p(out), 1, 257, 64, _p(long), 257) == INVALID


_MAIN = r"""
// stand-alone driver of csrc/abn_pack.cpp under the sanitizers: round trips with exactly sized heap buffers (an
// access one byte outside is a report), and the refusals
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "abneutral.h"

static unsigned long long state = 88172645463325252ull;
static unsigned rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (unsigned)(state >> 11); }
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
  const int ns[] = {1, 3, 17};
  const long long Ls[] = {0, 1, 15, 16, 17, 255, 256, 257, 1000};
  int trips = 0;
  for (int n : ns)
    for (long long L : Ls)
      for (long long extra : {0ll, 64ll}) {
        const long long src = L + 5, stride = abn_packed_row_stride(L) + extra;
        CHECK(stride % 64 == 0 && stride * 4 >= L);
        std::vector<unsigned char> codes((size_t)(n * src) + 1), packed((size_t)(n * stride) + 1), back((size_t)(n * L) + 1);
        for (auto& c : codes) { const unsigned r = rnd(); c = (unsigned char)((r & 8) ? (0x80 | (r >> 8)) : (r >> 4) % 3); }
        // the exact extents: the trailing byte of each vector is a canary outside what the functions may touch
        packed.back() = 0xA5; back.back() = 0x5A;
        CHECK(abn_pack_codes(codes.data(), n, L, src, packed.data(), stride) == ABN_OK);
        CHECK(abn_unpack_codes(packed.data(), n, L, stride, back.data(), L) == ABN_OK);
        CHECK(packed.back() == 0xA5 && back.back() == 0x5A);
        for (int s = 0; s < n; ++s) {
          for (long long k = 0; k < L; ++k) {
            const unsigned char c = codes[(size_t)(s * src + k)];
            CHECK(back[(size_t)(s * L + k)] == ((c & 0x80) ? 0x80 : c));
          }
          for (long long k = L; k < 4 * stride; ++k)   // the padding fields are 3
            CHECK(((packed[(size_t)(s * stride + (k >> 4) * 4 + (k & 3))] >> (2 * ((k >> 2) & 3))) & 3) == 3);
        }
        ++trips;
      }
  {  // exactly sized malloc blocks: nothing to spare on either side
    const long long L = 257, stride = 128;
    unsigned char* codes = (unsigned char*)std::malloc((size_t)L);
    unsigned char* packed = (unsigned char*)std::malloc((size_t)stride);
    std::memset(codes, 2, (size_t)L);
    CHECK(abn_pack_codes(codes, 1, L, L, packed, stride) == ABN_OK);
    CHECK(abn_unpack_codes(packed, 1, L, stride, codes, L) == ABN_OK);
    codes[256] = 3;
    CHECK(abn_pack_codes(codes, 1, L, L, packed, stride) == ABN_ERR_INVALID_ARG);
    codes[256] = 0x40;
    CHECK(abn_pack_codes(codes, 1, L, L, packed, stride) == ABN_ERR_INVALID_ARG);
    codes[256] = 0;
    CHECK(abn_pack_codes(codes, 1, L, L, packed, 32) == ABN_ERR_INVALID_ARG);
    CHECK(abn_pack_codes(codes, 1, L, L, packed, 64) == ABN_ERR_INVALID_ARG);
    CHECK(abn_pack_codes(codes, 1, L, L - 1, packed, stride) == ABN_ERR_INVALID_ARG);
    CHECK(abn_pack_codes(nullptr, 1, L, L, packed, stride) == ABN_ERR_INVALID_ARG);
    CHECK(abn_pack_codes(codes, 1, L, L, nullptr, stride) == ABN_ERR_INVALID_ARG);
    CHECK(abn_unpack_codes(nullptr, 1, L, stride, codes, L) == ABN_ERR_INVALID_ARG);
    CHECK(abn_unpack_codes(packed, 1, L, stride, nullptr, L) == ABN_ERR_INVALID_ARG);
    CHECK(abn_unpack_codes(packed, 1, L, 64, codes, L) == ABN_ERR_INVALID_ARG);
    CHECK(abn_packed_row_stride(0) == 0 && abn_packed_row_stride(1) == 64 && abn_packed_row_stride(256) == 64 &&
          abn_packed_row_stride(257) == 128 && abn_packed_row_stride(-5) == 0);
    std::free(codes);
    std::free(packed);
  }
  std::printf("sanitized pack ok %d\n", trips);
  return 0;
}
"""


def test_pack_translation_unit_under_address_and_ub_sanitizers(tmp_path):
    """csrc/abn_pack.cpp holds no HIP: g++ builds it with a main() of its own under ASan + UBSan; nothing is loaded into
    python."""
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is a requirement of the CPU tier (the oracle and this program are built with it)"
    main = tmp_path / "pack_main.cpp"
    main.write_text(_MAIN)
    exe = tmp_path / "pack_asan"
    r = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-I", str(ROOT / "include"), "-o", str(exe), str(main),
                        str(ROOT / "alphabeta_rs_amd" / "csrc" / "abn_pack.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sanitized pack ok 54" in r.stdout, r.stdout[-1500:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
