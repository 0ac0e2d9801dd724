// The window edges of the 2-bit packed codes (include/abneutral.h; src/pedigree.rs:210-261): which bits of one dword of
// sixteen fields to set so that the sites outside a column range read as 3 = filtered, and the sites per job of the
// packed windows scan (abn_pairwise_windows_packed.hpp).  Plain arithmetic, no HIP header: the kernel, the host's
// launch policy and the CPU tests (tests/test_pairwise_windows_packed_cpu.py) all include this file as it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ABN_HOST_DEVICE __host__ __device__
#else
#define ABN_HOST_DEVICE
#endif

namespace abn {

constexpr long long kPackedStepSites = 256;  // a super-step: 64 bytes of a row

// Sites per job of a chunked window on packed codes.  32 768 sites are 8 KiB of a row — what kPmxWinChunkSites = 8192
// byte codes are — so a job reads the same bytes per row against the same 32 KiB partial row as in the byte scan: a
// reasoned value (docs/experiments.md, "Packed windows").  A window's cuts are at b0 + k * chunk, b0 = its begin rounded
// down to 256 sites: every cut is a multiple of 256, so only a window's first and last job have a masked edge.
constexpr long long kPmxWinPackedChunkSites = 32768;
static_assert(kPmxWinPackedChunkSites % kPackedStepSites == 0 && kPmxWinPackedChunkSites < (1ll << 30),
              "whole super-steps; a job's packed 32-bit sums");

// the bits of the fields of the sites [0, t) of a dword, t in 0..16: site 4 j + e is byte e, bits 2j..2j+1
ABN_HOST_DEVICE inline uint32_t abn_packed_below(int t) {
  const int j = t >> 2, e = t & 3;
  const uint32_t whole = ((1u << (2 * j)) - 1u) * 0x01010101u;                            // the shifts below j, every byte
  const uint32_t part = ((3u << (2 * j)) & 0xffu) * (0x01010101u & ((1u << (8 * e)) - 1u));  // shift j, the bytes below e
  return whole | part;
}
// To keep the sites [lo, hi) of a dword's sixteen (0 <= lo <= hi <= 16): the bits that become 11, i. e. the fields of
// every other site.  dword | mask then reads as filtered outside [lo, hi) and is unchanged inside.
ABN_HOST_DEVICE inline uint32_t abn_packed_outside_mask(int lo, int hi) {
  return abn_packed_below(lo) | ~abn_packed_below(hi);
}
// ... for the dword whose first site is `site0`, of the column range [begin, end) of the row (all three counted from
// one origin that keeps them in an int, such as the first site of the dword's super-step)
ABN_HOST_DEVICE inline uint32_t abn_packed_window_mask(int site0, int begin, int end) {
  const int lo = begin - site0, hi = end - site0;
  const int l = lo < 0 ? 0 : (lo > 16 ? 16 : lo), h = hi < 0 ? 0 : (hi > 16 ? 16 : hi);
  return l < h ? abn_packed_outside_mask(l, h) : 0xffffffffu;
}

}  // namespace abn
