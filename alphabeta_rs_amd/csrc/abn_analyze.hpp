// RawAnalysis::analyze (src/analysis.rs:50-98) for every window of a device-resident bootstrap table in one launch:
// raw[W x B x 7] -> out[W x 32] (mean[8], sd[8], ci_lo[8], ci_hi[8]) and first_bad[W], every number with the bits of
// abn_analyze (abn_analyze.hip) on that window's table.  DESIGN.md §4 "Analysis".
//
// One workgroup of four wavefronts per (window, output column); the wavefronts never wait for one another until the one
// barrier at the end, each has a job of its own:
//   wavefront 0  the serial chains — the mean's fold (plain, or ndarray's eight accumulators for beta / alpha) and
//                Welford's standard deviation.  Their order of operations IS the result, so there is nothing to split:
//                the 64 lanes load (and, for beta / alpha, divide) 64 values at a time, then every lane runs the same
//                chain over them, one broadcast value after the other.
//   wavefront 1  the 0.025 quantile, wavefront 2 the 0.975 quantile: a most-significant-digit radix select of the order
//                statistic `lo` on 64-bit keys (abn_analyze_rank.hpp), eight passes over a 256-bin histogram in LDS, then
//                `hi` = lo + 1 from the count of keys equal to s[lo] and the smallest key above it.  No sort, no limit
//                on B, nothing kept per value.
//   wavefront 3  the NaN test of RawAnalysis::analyze over the window's rows: first_bad.
// The parallelism is the 8 W workgroups.  Compiled with -ffp-contract=off like everything else: the one fused
// multiply-add is Welford's, explicit, as in the reference's mul_add.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "abn_analyze_rank.hpp"

namespace abn {

constexpr int kAnWave = 64, kAnWaves = 4, kAnThreads = kAnWave * kAnWaves;
constexpr int kAnMaxWindowsPerLaunch = 1 << 24;  // 8 workgroups each: the grid stays below 2^31

struct AnalyzeArgs {
  const double* raw;   // [W x B x 7]
  double* out;         // [W x 32]
  int32_t* first_bad;  // [W]
  long long B;         // 1 .. 2^31 - 1
  int w0;              // first window of this launch
};

// value i of an output column of one window's table; cidx < 0: beta / alpha (src/analysis.rs:54), a true division
__device__ __forceinline__ double an_value(const double* tab, int cidx, long long i) {
  const double* row = tab + 7 * i;
  return cidx < 0 ? row[1] / row[0] : row[cidx];
}

// The lanes of ONE wavefront order their LDS traffic among themselves: the LDS serves a wavefront's instructions in
// order, so all that is needed is that the compiler keeps them in order too.  No s_barrier: the other wavefronts of the
// workgroup are elsewhere.
__device__ __forceinline__ void an_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// key of the order statistic `rank` (0-based, ascending) of the column, selected by one wavefront; *n_equal = how many
// values have that key, *rank_in_equal = the position of `rank` among them
__device__ __forceinline__ uint64_t an_select(const double* tab, int cidx, long long B, unsigned rank, unsigned* hist,
                                              int lane, unsigned* n_equal, unsigned* rank_in_equal) {
  uint64_t prefix = 0;
  unsigned count = 0;
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    for (int b = lane; b < 256; b += kAnWave) __hip_atomic_store(&hist[b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    an_wave_sync();
    for (long long i = lane; i < B; i += kAnWave) {
      const uint64_t key = abn_order_key(an_value(tab, cidx, i));
      // the digits above this pass's (none in the first pass) are the ones selected so far
      if (pass == 0 || (key >> (shift + 8)) == prefix)
        __hip_atomic_fetch_add(&hist[(unsigned)(key >> shift) & 255u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    an_wave_sync();
    // the bin that holds `rank`: lane l owns bins 4 l .. 4 l + 3; an inclusive scan of the lanes' totals
    const unsigned c0 = __hip_atomic_load(&hist[4 * lane + 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    const unsigned c1 = __hip_atomic_load(&hist[4 * lane + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    const unsigned c2 = __hip_atomic_load(&hist[4 * lane + 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    const unsigned c3 = __hip_atomic_load(&hist[4 * lane + 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    const unsigned tot = c0 + c1 + c2 + c3;
    unsigned inc = tot;
#pragma unroll
    for (int off = 1; off < kAnWave; off <<= 1) {
      const unsigned o = __shfl_up(inc, off, kAnWave);
      if (lane >= off) inc += o;
    }
    const unsigned exc = inc - tot;
    const bool mine = rank >= exc && rank < inc;  // one lane: the bins of this pass hold more than `rank` values
    unsigned bin = 0, below = exc, cnt = c0;
    const unsigned r = rank - exc;
    if (r >= c0) { bin = 1; below = exc + c0; cnt = c1; }
    if (r >= c0 + c1) { bin = 2; below = exc + c0 + c1; cnt = c2; }
    if (r >= c0 + c1 + c2) { bin = 3; below = exc + c0 + c1 + c2; cnt = c3; }
    const unsigned long long who = __ballot(mine);
    const int src = who ? __ffsll((long long)who) - 1 : 0;
    bin = __shfl(bin + 4u * (unsigned)lane, src, kAnWave);
    below = __shfl(below, src, kAnWave);
    count = __shfl(cnt, src, kAnWave);
    rank -= below;
    prefix = (prefix << 8) | bin;
    an_wave_sync();  // every lane has read its bins before the next pass clears them
  }
  *n_equal = count;
  *rank_in_equal = rank;
  return prefix;
}

// the smallest key above `key` in the column (all ones if there is none), by one wavefront
__device__ __forceinline__ uint64_t an_next_key(const double* tab, int cidx, long long B, uint64_t key, int lane) {
  uint64_t best = ~0ull;
  for (long long i = lane; i < B; i += kAnWave) {
    const uint64_t k = abn_order_key(an_value(tab, cidx, i));
    if (k > key && k < best) best = k;
  }
#pragma unroll
  for (int off = kAnWave / 2; off >= 1; off >>= 1) {
    const uint64_t o = __shfl_xor((unsigned long long)best, off, kAnWave);
    if (o < best) best = o;
  }
  return best;
}

__global__ __launch_bounds__(kAnThreads) void abn_analyze_kernel(const AnalyzeArgs a) {
  __shared__ double s_res[4];  // mean, sd, ci_lo, ci_hi of this (window, column)
  __shared__ int s_first_bad;
  __shared__ unsigned s_hist[2][256];
  const int lane = threadIdx.x & (kAnWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int w = a.w0 + (int)(blockIdx.x >> 3), k = (int)(blockIdx.x & 7);
  const long long B = a.B;
  const double* tab = a.raw + (size_t)w * (size_t)B * 7;
  const int cidx = abn_analyze_source_column(k);

  if (wave == 0) {
    // ---- mean and standard deviation: abn_analyze's chains, operation for operation
    double acc = 0.0, wmean = 0.0, sum_sq = 0.0;
    double part[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // (indexed by constants only: eight registers)
    double x = 0.0;
    long long last = 0;
    int n = 0;
    auto welford = [&](double v, long long i) {
      const double delta = v - wmean;
      wmean = wmean + delta / (double)(int)(i + 1);
      sum_sq = __builtin_fma(v - wmean, delta, sum_sq);
    };
    for (long long base = 0; base < B; base += kAnWave) {
      last = base;
      n = (int)(B - base < kAnWave ? B - base : kAnWave);
      x = lane < n ? an_value(tab, cidx, base + lane) : 0.0;
      for (int g = 0; g < (n >> 3); ++g) {  // whole groups of eight
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = __shfl(x, 8 * g + q, kAnWave);
        if (cidx < 0) {  // contiguous Array1: ndarray's eight-lane unrolled fold
#pragma unroll
          for (int q = 0; q < 8; ++q) part[q] = part[q] + v[q];
        } else {  // strided column view: plain fold
#pragma unroll
          for (int q = 0; q < 8; ++q) acc = acc + v[q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) welford(v[q], base + 8 * g + q);
      }
    }
    if (cidx < 0) {
      acc = acc + (part[0] + part[4]);
      acc = acc + (part[1] + part[5]);
      acc = acc + (part[2] + part[6]);
      acc = acc + (part[3] + part[7]);
    }
    for (int j = n & ~7; j < n; ++j) {  // the tail below a group of eight: values of the last load
      const double v = __shfl(x, j, kAnWave);
      acc = acc + v;
      welford(v, last + j);
    }
    if (lane == 0) {
      s_res[0] = acc / (double)(int)B;
      s_res[1] = __builtin_sqrt(sum_sq / ((double)(int)B - 1.0));
    }
  } else if (wave <= 2) {
    // ---- one quantile: the order statistics lo and hi (hi is lo or lo + 1), interpolated
    const QuantileRank qr = abn_quantile_rank(abn_analyze_quantile(wave - 1), B);
    unsigned n_equal = 0, rank_in_equal = 0;
    const uint64_t key_lo = an_select(tab, cidx, B, (unsigned)qr.lo, s_hist[wave - 1], lane, &n_equal, &rank_in_equal);
    uint64_t key_hi = key_lo;
    if (qr.hi != qr.lo && rank_in_equal + 1u >= n_equal) key_hi = an_next_key(tab, cidx, B, key_lo, lane);
    if (lane == 0)
      s_res[1 + wave] = abn_quantile_interpolate(abn_order_key_value(key_lo), abn_order_key_value(key_hi), qr.frac);
  } else {
    // ---- the first bootstrap whose row RawAnalysis::analyze refuses
    int fb = 0x7fffffff;
    for (long long i = lane; i < B; i += kAnWave)
      if (abn_analyze_row_is_bad(tab + 7 * i)) {
        fb = (int)i;
        break;
      }
#pragma unroll
    for (int off = kAnWave / 2; off >= 1; off >>= 1) {
      const int o = __shfl_xor(fb, off, kAnWave);
      fb = o < fb ? o : fb;
    }
    if (lane == 0) s_first_bad = fb == 0x7fffffff ? -1 : fb;
  }
  __syncthreads();  // the only barrier, reached by every thread
  if (threadIdx.x == 0) {
    const bool bad = s_first_bad >= 0;
    double* o = a.out + (size_t)w * 32 + (size_t)k;
#pragma unroll
    for (int s = 0; s < 4; ++s) o[8 * s] = bad ? __builtin_nan("") : s_res[s];
    if (k == 0) a.first_bad[w] = s_first_bad;
  }
}

}  // namespace abn
