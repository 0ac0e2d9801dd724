// Pairwise divergence of MANY column ranges ("windows") of one 2-bit PACKED code matrix in one batch — the window loop of
// src/cli/metaprofile.rs:50-72 around DMatrix::from (src/pedigree.rs:210-261): the job model of abn_pairwise_windows.hpp
// (PairWinJob / PairWinTask, direct jobs and partial rows, abn_pairwise_win_reduce_kernel) on the packed front end of
// abn_pairwise_packed.hpp (PmxScan<NB, DIAG, true, PmxPackedCodes>).
//
// A window needs no shifting.  Both operands of every Gram product use the same assignment of sites to k slots and the
// sums are integers, so a job [begin, end) simply covers the aligned super-steps (64 bytes = 256 sites of every row)
// floor(begin / 256) .. ceil(end / 256) - 1 and reads the fields before `begin` and from `end` on as 3 (filtered).
// Every load is an aligned 16-byte load inside the row: no funnel-shift loader, no AL4 variants, no byte loads.
//
// Edges.  The front and the back super-step of a job — at most two, one where begin and end share a super-step — are
// loaded and dealt to the wavefronts like every other step of the job and masked IN REGISTERS inside the pipelined path:
// PmxScan::inner_steps hands every batch to the kernel's `fix` just before its matrix steps, and on the two edge steps
// (a scalar compare per step otherwise) the fragments are ORed with a per-dword mask (abn_packed_window_mask,
// abn_packed_mask.hpp) that sets the fields outside the job to 3.  No serial edge step behind the loop: a metaprofile
// window of 3000 sites is 12 super-steps, three per wavefront, and two more on the last wavefront, as the byte kernel
// runs them, would be two of five on the job's critical path.  (A masked step with matrix-step code of its own took the
// off-diagonal kernel, which has four registers to spare, to scratch memory.)
#pragma once
#include "abn_packed_mask.hpp"
#include "abn_pairwise_packed.hpp"
#include "abn_pairwise_windows.hpp"

namespace abn {

// The `fix` of a job [begin, end) on packed rows (Scan: the kernel's PmxScan; q: the lane's quarter of a step).
// Super-steps [s0(), s1()) of every row; the first and the last of them are masked where the job does not fill them.
template <class Scan>
struct PmxPackedWindowFix {
  long long begin, end;
  int q;
  __device__ __forceinline__ long long s0() const { return begin / kPackedStepSites; }
  __device__ __forceinline__ long long s1() const { return (end + kPackedStepSites - 1) / kPackedStepSites; }
  __device__ __forceinline__ void operator()(long long k, pmx_u32x4 (&x)[Scan::NF]) const {
    // ... counted from s0 (a job is below 2^30 sites: an int), -1: no such step
    const int kf = begin % kPackedStepSites != 0 ? 0 : -1;
    const int kb = end % kPackedStepSites != 0 ? (int)(s1() - 1 - s0()) : -1;
    // a step belongs to one wavefront: the compare is made on scalars, the branch around the masking is a scalar one
    const int ks = __builtin_amdgcn_readfirstlane((int)(k - s0()));
    if (ks != kf && ks != kb) return;
    // the job's range counted from the super-step's first site and clamped to the step; this lane's 16 bytes hold the
    // sites from 64 q on, 16 per dword
    const long long first = (s0() + ks) * kPackedStepSites, lo64 = begin - first, hi64 = end - first;
    const int lo = lo64 < 0 ? 0 : (int)lo64, hi = hi64 > kPackedStepSites ? (int)kPackedStepSites : (int)hi64;
#pragma unroll
    for (int d = 0; d < 4; ++d) {  // (a dword at a time: one mask register)
      const uint32_t m = abn_packed_window_mask(64 * q + 16 * d, lo, hi);
#pragma unroll
      for (int f = 0; f < Scan::NF; ++f) x[f][d] |= m;
    }
  }
};

// a.codes: the packed rows; a.row_stride: bytes per row (a multiple of 64 from a 16-byte aligned base); the jobs' begin
// and end are sites, end <= 4 row_stride
template <int NB, bool DIAG>
__global__ __launch_bounds__(kPmxThreads, DIAG ? 2 : 1) void abn_pairwise_win_packed_kernel(const PairWinArgs a) {
  using Scan = PmxScan<NB, DIAG, true, PmxPackedCodes>;
  __shared__ unsigned long long red[kPmxJobElems];
  Scan sc(a.codes);
  sc.wave = __builtin_amdgcn_readfirstlane(sc.wave);  // the step indices below: scalar registers, scalar branches
  const PairWinJob job = a.jobs[blockIdx.x];
  int R, C;
  if constexpr (DIAG) R = C = job.sp;
  else pmx_offdiag(job.sp, a.ngroups, R, C);
#pragma unroll
  for (int b = 0; b < Scan::NF; ++b) {
    const int blk = b < 4 ? 4 * R + b : 4 * C + (b - 4);
    int s = 16 * blk + sc.r;
    s = s < a.n ? s : a.n - 1;  // rows past n give sums nobody reads
    sc.roff[b] = (size_t)s * (size_t)a.row_stride;
  }

  PmxPackedWindowFix<Scan> mask_edges{job.begin, job.end, sc.q};
  sc.inner_steps(mask_edges.s0(), mask_edges.s1(), red, mask_edges);
  // (an empty job that does not sit on a step boundary reads one step and masks all of it: its sums stay zero)

  __syncthreads();
  sc.fold(red);
  __syncthreads();
  pmx_win_store<Scan>(a, job, R, C, red, sc.tid);
}

}  // namespace abn
