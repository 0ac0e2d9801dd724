// Window placement of methylome sites on the device (abn_windows_*): the part of Windows::extract
// (src/windows.rs:287-343) behind the gene choice — MethylationSite::place_in_windows (src/methylation_site.rs:423-490)
// for every site of every sample, the per-window site lists in file order, the 2-bit packed matrix that
// abn_pairwise_divergence_windows_packed scans (layout: host/pedigree_build.hpp, layout_packed_call) and the folds of
// Windows::steady_state_methylation (src/windows.rs:94-128) and of the pedigree's rc_meth_lvl (src/pedigree.rs:165-166).
//
//   K1 abn_windows_place_kernel    one site per lane: the interval [lo, hi] of global window indices it is pushed to
//   K2 abn_windows_rank_kernel     a workgroup per block of kWinBlockSites sites of ONE sample, a lane per window bin:
//                                  the lane walks the block's intervals in file order (one LDS broadcast per site), so
//                                  its running count IS the stable in-block rank.  Pass 0 writes the bin's count of the
//                                  block, pass 1 (after the scan) writes the site indices to their slots of the lists
//      abn_windows_scan_kernel     a lane per (sample, window): exclusive scan of the bin's counts over the sample's blocks
//   K3 abn_windows_pack_kernel     a lane per dword of the packed matrix: 16 sites gathered through the list
//   K4 abn_windows_sums_kernel     a lane per (sample, window): serial folds in list order
// Every output element has exactly one writer and is written with a plain vector store; there are no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace abn {

constexpr int kWinThreads = 256;
constexpr int kWinBlockSites = 1024;  // sites per rank block: 8 KiB of LDS (lo, hi as int32)

struct WinParams {  // abn_windows_params, the region offsets resolved
  double cutoff, step, size;
  int absolute;
  int n_region[3];  // windows of upstream, gene, downstream (Windows::new, src/windows.rs:28-44)
  int first[3];     // global index of each region's window 0
  int W;
};

struct WinBlock {  // a rank block: sites [site0, site0 + len) of `sample`
  long long site0;
  int len, sample;
};

// src/methylation_site.rs:480-488 — the bounds of window i, in the reference's operation order
__device__ __forceinline__ double win_lower(int i, double step) { return (double)i * step - 0.1; }
__device__ __forceinline__ double win_upper(int i, double step, double size) { return win_lower(i, step) + size + 0.1; }

// place_in_windows for one site: the global indices [lo, hi] of the windows it is pushed to (lo > hi: none).  Both bounds
// are non-decreasing in i, so the windows with lower <= position are a prefix and those with upper >= position a suffix
// of the region: the interval is found from an arithmetic guess and settled with the reference's own comparisons.
__device__ __forceinline__ void win_place(uint32_t pos, uint32_t gstart, uint32_t gend, uint8_t flags, const WinParams& P,
                                          int& lo_out, int& hi_out) {
  lo_out = 0;
  hi_out = -1;
  if (!(flags & 2)) return;  // no gene (src/windows.rs:334)
  const double location = (double)pos, cutoff = P.cutoff, step = P.step, size = P.size;
  const double start = (double)gstart, end = (double)gend, length = end - start;
  const bool anti = flags & 1;  // Unknown was placed as Sense (:439-443)
  const double offset = anti ? end - location : location - start;
  const int region = offset < 0.0 ? 0 : (offset > length ? 2 : 1);
  double position;
  if (!anti) position = region == 0 ? location - start + cutoff : (region == 1 ? location - start : location - end);
  else position = region == 0 ? end - location + cutoff : (region == 1 ? end - location : start - location);
  if (!P.absolute) {
    position = region == 1 ? position / length : position / cutoff;
    position *= 100.0;
  }
  const int n = P.n_region[region];
  if (!(position == position) || n <= 0) return;  // NaN (a gene of length 0) is in no window
  const double gh = (position + 0.1) / step, gl = (position - size - 0.2) / step;
  int hi = gh >= (double)n ? n - 1 : (gh < 0.0 ? -1 : (int)gh);
  int lo = gl >= (double)n ? n : (gl < 0.0 ? 0 : (int)gl);
  while (hi + 1 < n && position >= win_lower(hi + 1, step)) ++hi;
  while (hi >= 0 && !(position >= win_lower(hi, step))) --hi;
  while (lo > 0 && position <= win_upper(lo - 1, step, size)) --lo;
  while (lo < n && !(position <= win_upper(lo, step, size))) ++lo;
  if (lo > hi) return;
  lo_out = P.first[region] + lo;
  hi_out = P.first[region] + hi;
}

// K1
__global__ void __launch_bounds__(kWinThreads)
abn_windows_place_kernel(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ gstart,
                         const uint32_t* __restrict__ gend, const uint8_t* __restrict__ flags, long long n_sites,
                         WinParams P, int2* __restrict__ span) {
  const long long i = (long long)blockIdx.x * kWinThreads + threadIdx.x;
  if (i >= n_sites) return;
  int lo, hi;
  win_place(pos[i], gstart[i], gend[i], flags[i], P, lo, hi);
  span[i] = make_int2(lo, hi);
}

// K2, both passes.  hist[w * n_blocks + b]: pass 0 writes the number of sites of block b in window w; the scan turns it
// into the rank of the block's first such site inside (sample, w); pass 1 reads that and fills the list.
// list_off[sample * W + w]: where the list of (sample, w) starts in `list`; entries are site indices inside the sample.
template <int PASS>
__global__ void __launch_bounds__(kWinThreads)
abn_windows_rank_kernel(const int2* __restrict__ span, const WinBlock* __restrict__ blocks, int n_blocks, int W,
                        uint32_t* __restrict__ hist, const long long* __restrict__ list_off,
                        const long long* __restrict__ sample_site0, uint32_t* __restrict__ list) {
  __shared__ int2 s_span[kWinBlockSites];
  const WinBlock blk = blocks[blockIdx.x];
  for (int t = threadIdx.x; t < blk.len; t += kWinThreads) s_span[t] = span[blk.site0 + t];
  __syncthreads();
  const uint32_t local0 = (uint32_t)(blk.site0 - sample_site0[blk.sample]);
  for (int w = threadIdx.x; w < W; w += kWinThreads) {
    const size_t h = (size_t)w * (size_t)n_blocks + blockIdx.x;
    uint32_t k = 0;
    if (PASS == 0) {
      for (int t = 0; t < blk.len; ++t) {
        const int2 s = s_span[t];
        k += (s.x <= w && w <= s.y) ? 1u : 0u;
      }
      hist[h] = k;
    } else {
      uint32_t* out = list + list_off[(size_t)blk.sample * W + w] + hist[h];
      for (int t = 0; t < blk.len; ++t) {
        const int2 s = s_span[t];
        if (s.x <= w && w <= s.y) out[k++] = local0 + (uint32_t)t;
      }
    }
  }
}

// the scan over blocks per bin: lane (sample, w) walks the sample's blocks [block0[sample], block0[sample + 1])
__global__ void __launch_bounds__(kWinThreads)
abn_windows_scan_kernel(uint32_t* __restrict__ hist, const int* __restrict__ block0, int n_blocks, int n_samples, int W,
                        long long* __restrict__ count) {
  const long long i = (long long)blockIdx.x * kWinThreads + threadIdx.x;
  if (i >= (long long)n_samples * W) return;
  const int s = (int)(i / W), w = (int)(i % W);
  uint32_t run = 0;
  for (int b = block0[s]; b < block0[s + 1]; ++b) {
    const size_t h = (size_t)w * (size_t)n_blocks + (size_t)b;
    const uint32_t c = hist[h];
    hist[h] = run;
    run += c;
  }
  count[i] = (long long)run;
}

// K3.  col0[w] (W + 1 entries, in dwords): where window w's columns begin in every row — a multiple of 16 dwords; a
// ragged window has col0[w + 1] == col0[w].  A field beyond the window's sites, and every dword behind the last window,
// is 3.  Field of site 16 g + 4 j + e: byte e of dword g, bits 2j..2j+1 (include/abneutral.h, abn_pack_codes).
__global__ void __launch_bounds__(kWinThreads)
abn_windows_pack_kernel(const uint8_t* __restrict__ code, const uint32_t* __restrict__ list,
                        const long long* __restrict__ list_off, const long long* __restrict__ count,
                        const long long* __restrict__ sample_site0, const long long* __restrict__ col0, int W,
                        int n_samples, long long row_dwords, uint32_t* __restrict__ packed) {
  const long long i = (long long)blockIdx.x * kWinThreads + threadIdx.x;
  if (i >= (long long)n_samples * row_dwords) return;
  const int s = (int)(i / row_dwords);
  const long long d = i % row_dwords;
  uint32_t out = 0xffffffffu;
  if (d < col0[W]) {
    int a = 0, b = W;  // the last w with col0[w] <= d; windows without columns share their successor's col0
    while (b - a > 1) {
      const int m = (a + b) >> 1;
      if (col0[m] <= d) a = m; else b = m;
    }
    const long long first = (d - col0[a]) * 16, n = count[(size_t)s * W + a];
    const uint32_t* l = list + list_off[(size_t)s * W + a];
    const uint8_t* c = code + sample_site0[s];
    out = 0;
    for (int k = 0; k < 16; ++k) {
      uint32_t f = 3u;
      if (first + k < n) {
        const uint8_t v = c[l[first + k]];
        f = (v & 0x80u) ? 3u : (uint32_t)(v & 3u);
      }
      out |= f << (8 * (k & 3) + 2 * (k >> 2));
    }
  }
  packed[i] = out;
}

// K4: the folds `acc + cur.meth_lvl` from 0.0 in push order (src/windows.rs:94-128) and, over the sites whose posterior
// passes the filter, the sum and count of src/pedigree.rs:165-166
__global__ void __launch_bounds__(kWinThreads)
abn_windows_sums_kernel(const uint8_t* __restrict__ code, const double* __restrict__ level,
                        const uint32_t* __restrict__ list, const long long* __restrict__ list_off,
                        const long long* __restrict__ count, const long long* __restrict__ sample_site0, int W,
                        int n_samples, double* __restrict__ level_sum, double* __restrict__ level_sum_kept,
                        long long* __restrict__ kept) {
  const long long i = (long long)blockIdx.x * kWinThreads + threadIdx.x;
  if (i >= (long long)n_samples * W) return;
  const int s = (int)(i / W);
  const uint32_t* l = list + list_off[i];
  const long long n = count[i], base = sample_site0[s];
  double all = 0.0, sum = 0.0;
  long long k = 0;
  for (long long j = 0; j < n; ++j) {
    const long long site = base + l[j];
    const double v = level[site];
    all = all + v;
    if (code[site] < 0x80) {
      sum = sum + v;
      ++k;
    }
  }
  level_sum[i] = all;
  level_sum_kept[i] = sum;
  kept[i] = k;
}

}  // namespace abn
