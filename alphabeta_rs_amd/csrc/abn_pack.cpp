// The 2-bit packed code format of the pairwise scan (src/pedigree.rs:210-261; include/abneutral.h): host arithmetic
// only — no HIP in this translation unit, so that it also builds alone under the host sanitizers
// (tests/test_pairwise_packed_cpu.py).  The kernel that reads the format is in abn_pairwise_packed.hpp.
#include <stddef.h>

#include "../../include/abneutral.h"

namespace {
// site k of a row -> its byte in the row and the shift of its field there: site 16 g + 4 j + e is byte e of dword g
// (little-endian), bits 2j..2j+1
inline size_t field_byte(size_t k) { return (k >> 4) * 4 + (k & 3); }
inline unsigned field_shift(size_t k) { return 2u * (unsigned)((k >> 2) & 3); }

bool stride_ok(int64_t n_sites, int64_t row_stride_bytes) {
  return row_stride_bytes >= 0 && row_stride_bytes % 64 == 0 && row_stride_bytes >= abn_packed_row_stride(n_sites);
}
}  // namespace

extern "C" int64_t abn_packed_row_stride(int64_t n_sites) {
  return n_sites <= 0 ? 0 : (n_sites + 255) / 256 * 64;  // whole super-steps of 256 sites = 64 bytes
}

extern "C" int abn_pack_codes(const uint8_t* codes, int32_t n_samples, int64_t n_sites, int64_t src_row_stride,
                              uint8_t* packed, int64_t row_stride_bytes) {
  if (!codes || !packed || n_samples < 0 || n_sites < 0 || src_row_stride < n_sites) return ABN_ERR_INVALID_ARG;
  if (!stride_ok(n_sites, row_stride_bytes)) return ABN_ERR_INVALID_ARG;
  const size_t L = (size_t)n_sites, stride = (size_t)row_stride_bytes;
  for (size_t s = 0; s < (size_t)n_samples; ++s) {
    const uint8_t* src = codes + s * (size_t)src_row_stride;
    uint8_t* dst = packed + s * stride;
    for (size_t b = 0; b < stride; ++b) dst[b] = 0xff;  // the padding: every field from site L on is 3
    for (size_t k = 0; k < L; ++k) {
      const uint8_t c = src[k];
      if (!(c & 0x80) && c > 2) return ABN_ERR_INVALID_ARG;  // not a code: 0, 1, 2 or 0x80 | anything
      const unsigned f = (c & 0x80) ? 3u : c;
      dst[field_byte(k)] ^= (uint8_t)((3u ^ f) << field_shift(k));  // the field was 3
    }
  }
  return ABN_OK;
}

extern "C" int abn_unpack_codes(const uint8_t* packed, int32_t n_samples, int64_t n_sites, int64_t row_stride_bytes,
                                uint8_t* codes, int64_t dst_row_stride) {
  if (!codes || !packed || n_samples < 0 || n_sites < 0 || dst_row_stride < n_sites) return ABN_ERR_INVALID_ARG;
  if (!stride_ok(n_sites, row_stride_bytes)) return ABN_ERR_INVALID_ARG;
  for (size_t s = 0; s < (size_t)n_samples; ++s) {
    const uint8_t* src = packed + s * (size_t)row_stride_bytes;
    uint8_t* dst = codes + s * (size_t)dst_row_stride;
    for (size_t k = 0; k < (size_t)n_sites; ++k) {
      const unsigned f = (src[field_byte(k)] >> field_shift(k)) & 3u;
      dst[k] = f == 3u ? (uint8_t)0x80 : (uint8_t)f;
    }
  }
  return ABN_OK;
}
