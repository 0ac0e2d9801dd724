// The state census of a 2-bit packed code matrix per column range ("window"): how many fields 0, 1 and 2 — U, I, M of
// src/pedigree.rs:253-257 — every sample keeps inside [begin, end).  rc_meth_lvl of a sample is a mean over the sample's
// OWN kept sites (src/pedigree.rs:159-175); the pair tables of abn_pairwise_transitions.hpp only know the sites both
// samples of a pair keep, so they cannot give it once sites drop out of single samples.  Plain arithmetic, no HIP header:
// the serial form, the job plan and the walk of the kernel's lane structure compile with a host compiler
// (tests/native/sim_study_main.cpp); the kernels only where abn_pairwise.hip asks for them (ABN_CENSUS_KERNELS).
//
// MAPPING.  A job is a chunk of a window; a workgroup runs one job of one sample (grid: jobs on x, samples on y).  The
// cuts are the packed windows scan's: chunk sites (kPmxWinPackedChunkSites, more only where that scan takes more) counted
// from the window's begin rounded down to 256 sites, so every cut is a multiple of 256, only a window's first and last
// job have an edge, and every load is an aligned 16-byte load inside the row.  The edges are masked with
// abn_packed_window_mask: a field outside the job reads as 3.  Per dword x: lo = x & 0x55555555, hi = (x >> 1) &
// 0x55555555; the fields 0 are the bits of ~(lo | hi) & 0x55555555, the fields 1 those of lo & ~hi, the fields 2 those of
// hi & ~lo.  A lane sums the population counts of its 16-byte loads, the workgroup reduces them — wavefront by shuffles,
// the four wavefronts through kCensusRedWords words of LDS — to three 32-bit partials, which a job of fewer than 2^30
// sites cannot overflow.  A second kernel sums the partials of every (window, sample) into 64 bits: one wavefront each,
// the lanes strided over the window's jobs.  No atomics: integer sums, independent of the launch.  An empty window has no
// job and gets zeros from the second kernel.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "abn_packed_mask.hpp"

namespace abn {

constexpr int kCensusThreads = 256;                          // four wavefronts
constexpr int kCensusRedWords = 3 * (kCensusThreads / 64);   // the LDS of a workgroup: three counts per wavefront
constexpr int kCensusSumThreads = 64;                        // the second kernel: one wavefront per (window, sample)

struct CensusJob {
  long long begin, end;  // sites, begin < end; begin is a multiple of 256 unless it is the window's, end likewise
};

// the counts of the fields 0, 1, 2 of a dword
ABN_HOST_DEVICE inline void census_dword(uint32_t x, uint32_t& n0, uint32_t& n1, uint32_t& n2) {
  const uint32_t lo = x & 0x55555555u, hi = (x >> 1) & 0x55555555u;
  n0 += (uint32_t)__builtin_popcount(~(lo | hi) & 0x55555555u);
  n1 += (uint32_t)__builtin_popcount(lo & ~hi);
  n2 += (uint32_t)__builtin_popcount(hi & ~lo);
}

// What one lane adds for the 16-byte load `q` (counted from the job's first super-step) of its job's row: the four
// dwords w[0..3], masked where q lies in the job's first or last super-step.  nq: the job's 16-byte loads
ABN_HOST_DEVICE inline void census_lane_quad(const CensusJob job, long long q, long long nq, const uint32_t w[4], uint32_t& n0,
                                             uint32_t& n1, uint32_t& n2) {
  const bool edge = q < 4 || q >= nq - 4;  // a super-step is four loads
  const long long first = job.begin / kPackedStepSites * kPackedStepSites;
  const int lo = (int)(job.begin - first), hi = (int)(job.end - first);  // a job is below 2^30 sites
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int d = 0; d < 4; ++d) {
    uint32_t x = w[d];
    if (edge) x |= abn_packed_window_mask((int)(64 * q + 16 * d), lo, hi);
    census_dword(x, n0, n1, n2);
  }
}
// the 16-byte loads of a job: whole super-steps from the one that holds begin to the one that holds end - 1
ABN_HOST_DEVICE inline long long census_job_quads(const CensusJob job) {
  return ((job.end + kPackedStepSites - 1) / kPackedStepSites - job.begin / kPackedStepSites) * 4;
}

// The jobs of W windows (valid ranges; chunk[w]: the sites per job of window w, a multiple of 256): window w's jobs are
// jobs[job_off[w] .. job_off[w + 1])
inline void census_plan(const int64_t* begin, const int64_t* end, int64_t W, const long long* chunk, std::vector<CensusJob>& jobs,
                        std::vector<long long>& job_off) {
  jobs.clear();
  job_off.assign((size_t)W + 1, 0);
  for (int64_t w = 0; w < W; ++w) {
    const long long b0 = begin[w] - begin[w] % kPackedStepSites;
    for (long long at = b0; at < end[w] && begin[w] < end[w]; at += chunk[w])
      jobs.push_back(CensusJob{at < begin[w] ? (long long)begin[w] : at, at + chunk[w] < end[w] ? at + chunk[w] : (long long)end[w]});
    job_off[(size_t)w + 1] = (long long)jobs.size();
  }
}

// "" or why the arguments are refused, in the words of the packed windows scan's checks (abn_pairwise.hip)
inline std::string census_refusal(const void* packed, int64_t n, int64_t n_sites, int64_t row_stride, const int64_t* begin,
                                  const int64_t* end, int64_t W, const void* counts) {
  if (!packed || n <= 0 || n_sites < 0) return "null/size";
  if (row_stride < 0 || row_stride % 64 != 0 || row_stride < (n_sites + 255) / 256 * 64)
    return "row_stride_bytes is not a multiple of 64 that holds n_sites fields";
  if (n > 65535) return "too many samples";
  if (W < 0 || (W > 0 && (!begin || !end || !counts))) return "null/size";
  for (int64_t w = 0; w < W; ++w)
    if (begin[w] < 0 || begin[w] > end[w] || end[w] > n_sites)
      return "window " + std::to_string(w) + " is not a column range of the rows";
  return "";
}

// The serial form, field by field: counts uint64 [W x n x 3]
inline void census_windows_serial(const uint8_t* packed, int64_t n, int64_t row_stride, const int64_t* begin, const int64_t* end,
                                  int64_t W, uint64_t* counts) {
  for (int64_t w = 0; w < W; ++w)
    for (int64_t s = 0; s < n; ++s) {
      uint64_t c[4] = {0, 0, 0, 0};
      const uint8_t* row = packed + s * row_stride;
      for (int64_t k = begin[w]; k < end[w]; ++k) ++c[(row[(k >> 4) * 4 + (k & 3)] >> (2 * ((k >> 2) & 3))) & 3];
      for (int f = 0; f < 3; ++f) counts[(w * n + s) * 3 + f] = c[f];
    }
}

// The kernels' structure walked on the host: every job's workgroup of kCensusThreads lanes strided over the job's 16-byte
// loads into partial [n x jobs x 3], then every (window, sample)'s sum of its jobs' partials
inline void census_windows_walk(const uint8_t* packed, int64_t n, int64_t row_stride, const int64_t* begin, const int64_t* end,
                                int64_t W, const long long* chunk, uint64_t* counts) {
  std::vector<CensusJob> jobs;
  std::vector<long long> job_off;
  census_plan(begin, end, W, chunk, jobs, job_off);
  const size_t J = jobs.size();
  std::vector<uint32_t> partial((size_t)n * J * 3 + 1, 0);
  for (size_t j = 0; j < J; ++j)
    for (int64_t s = 0; s < n; ++s) {
      const long long nq = census_job_quads(jobs[j]), q0 = jobs[j].begin / kPackedStepSites * 4;
      uint32_t sum[3] = {0, 0, 0};
      for (int lane = 0; lane < kCensusThreads; ++lane) {
        uint32_t n0 = 0, n1 = 0, n2 = 0;
        for (long long q = lane; q < nq; q += kCensusThreads) {
          uint32_t w4[4];
          const uint8_t* at = packed + s * row_stride + 16 * (q0 + q);
          for (int d = 0; d < 4; ++d)
            w4[d] = (uint32_t)at[4 * d] | (uint32_t)at[4 * d + 1] << 8 | (uint32_t)at[4 * d + 2] << 16 | (uint32_t)at[4 * d + 3] << 24;
          census_lane_quad(jobs[j], q, nq, w4, n0, n1, n2);
        }
        sum[0] += n0, sum[1] += n1, sum[2] += n2;
      }
      for (int f = 0; f < 3; ++f) partial[((size_t)s * J + j) * 3 + (size_t)f] = sum[f];
    }
  for (int64_t w = 0; w < W; ++w)
    for (int64_t s = 0; s < n; ++s)
      for (int f = 0; f < 3; ++f) {
        uint64_t total = 0;
        for (long long j = job_off[(size_t)w]; j < job_off[(size_t)w + 1]; ++j) total += partial[((size_t)s * J + (size_t)j) * 3 + (size_t)f];
        counts[(w * n + s) * 3 + f] = total;
      }
}

#if defined(__HIPCC__) && defined(ABN_CENSUS_KERNELS)  // (abn_pairwise.hip defines it)
// grid (a slab of jobs from j_base, n) of kCensusThreads lanes; packed: 16-byte aligned, row_stride a multiple of 64.
// Bounds: a job's loads end at the super-step that holds its end - 1, and end <= n_sites <= 4 row_stride; blockIdx.y < n;
// j_base + blockIdx.x < J; partial [n x J x 3].
__global__ void __launch_bounds__(kCensusThreads)
abn_packed_census_kernel(const uint8_t* __restrict__ packed, long long row_stride, const CensusJob* __restrict__ jobs,
                         long long J, long long j_base, uint32_t* __restrict__ partial) {
  __shared__ uint32_t red[kCensusRedWords];
  const long long j = j_base + blockIdx.x;
  const CensusJob job = jobs[j];
  const long long nq = census_job_quads(job), q0 = job.begin / kPackedStepSites * 4;
  const uint4* row = reinterpret_cast<const uint4*>(packed + (size_t)blockIdx.y * (size_t)row_stride) + q0;
  uint32_t n0 = 0, n1 = 0, n2 = 0;
  for (long long q = threadIdx.x; q < nq; q += kCensusThreads) {
    const uint4 x = row[q];
    const uint32_t w4[4] = {x.x, x.y, x.z, x.w};
    census_lane_quad(job, q, nq, w4, n0, n1, n2);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n0 += __shfl_down(n0, off, 64);
    n1 += __shfl_down(n1, off, 64);
    n2 += __shfl_down(n2, off, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[3 * wave + 0] = n0, red[3 * wave + 1] = n1, red[3 * wave + 2] = n2;
  __syncthreads();
  if (threadIdx.x < 3) {
    uint32_t sum = 0;
#pragma unroll
    for (int w = 0; w < kCensusThreads / 64; ++w) sum += red[3 * w + threadIdx.x];
    partial[((size_t)blockIdx.y * (size_t)J + (size_t)j) * 3 + threadIdx.x] = sum;
  }
}

// grid (a slab of windows from w_base, n) of kCensusSumThreads lanes: counts[(w n + s) 3 + f] = the sum over the window's
// jobs; J: all jobs; job_off [W + 1]
__global__ void __launch_bounds__(kCensusSumThreads)
abn_packed_census_sum_kernel(const uint32_t* __restrict__ partial, const long long* __restrict__ job_off, long long J,
                             long long w_base, unsigned long long* __restrict__ counts) {
  const long long w = w_base + blockIdx.x;
  const long long j0 = job_off[w], j1 = job_off[w + 1];
  const uint32_t* p = partial + (size_t)blockIdx.y * (size_t)J * 3;
  unsigned long long c0 = 0, c1 = 0, c2 = 0;
  for (long long j = j0 + threadIdx.x; j < j1; j += kCensusSumThreads) c0 += p[3 * j], c1 += p[3 * j + 1], c2 += p[3 * j + 2];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    c0 += __shfl_down(c0, off, 64);
    c1 += __shfl_down(c1, off, 64);
    c2 += __shfl_down(c2, off, 64);
  }
  if (threadIdx.x == 0) {
    unsigned long long* out = counts + ((size_t)w * gridDim.y + blockIdx.y) * 3;
    out[0] = c0, out[1] = c1, out[2] = c2;
  }
}
#endif

}  // namespace abn
