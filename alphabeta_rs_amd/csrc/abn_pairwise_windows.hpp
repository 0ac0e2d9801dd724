// Pairwise divergence of MANY column ranges ("windows") of one code matrix in one batch — the window loop of
// src/cli/metaprofile.rs:50-72 around DMatrix::from (src/pedigree.rs:210-261) as one device job.  The arithmetic, the
// loaders and the register pipeline are those of abn_pairwise_mx.hpp (PmxScan); what is new is the job and its edges.
//
// A job = (window, super-pair of 64-sample groups, site chunk), described by one PairWinJob the host writes.  A window of
// at most kPmxWinChunkSites sites is ONE job per super-pair: its workgroup folds the four wavefronts' tiles in LDS and
// writes diff / both / dvalue of the window itself — no partial row, no second launch.  Longer windows are cut into
// chunks of that many sites (a multiple of 128: whole cache lines of an aligned row per batch); their jobs write packed
// partial rows as abn_pairwise_mx_kernel does and abn_pairwise_win_reduce_kernel sums them per (window, super-pair).
//
// Edges.  K steps count from the job's first site, so the front of a window is never ragged: the per-lane funnel-shift
// loader (pmx_load<false>) takes any byte address and reads the aligned dword that holds the first byte.  The back is:
// the steps that are not wholly inside [begin, end) with the loader's four bytes to spare before the END OF THE ROW —
// at most two per job — are taken one at a time by the job's last wavefront.  Where the row still holds the step's 64
// bytes (+ 4) the fragment is loaded as usual and the bytes from `end` on are replaced by 0x80 (filtered); only where
// the row itself ends first (the last row ends the caller's buffer) the bytes are loaded one by one (pmx_load_edge).
#pragma once
#include "abn_pairwise_mx.hpp"

namespace abn {

// Sites per job.  Smaller jobs balance better (a 200 000-site window next to 20 000-site ones would otherwise be the
// launch's critical path: one workgroup streams at a small fraction of the HBM rate) and cost one 32 KiB partial row
// each at most; 8192 sites are 128 K steps, 32 per wavefront — eight times the floor of four that the single-window
// launch policy keeps (abn_pairwise.hip) — and 0.5 MiB of codes per job of 64 samples against that row: 6 %.  Windows
// of a metaprofile run (a few thousand sites) stay below it and take the single-launch form.  Far below 2^30, the
// limit of a job's packed 32-bit sums.
constexpr long long kPmxWinChunkSites = 8192;
static_assert(kPmxWinChunkSites % 128 == 0 && kPmxWinChunkSites < (1ll << 30), "whole line pairs; 32-bit halves");

struct PairWinJob {
  long long begin, end;  // the job's sites [begin, end) of every row
  long long window;      // whose block of the outputs (direct jobs)
  int sp;                // super-pair: DIAG: group R = C = sp; else index among the pairs R < C as pmx_offdiag counts them
  int slot;              // row of `partial` (of this launch), or -1: the job is its window's only one and writes the result
};
struct PairWinTask {     // one (window, super-pair) of a chunked window: rows [row0, row0 + nchunks) of `partial`
  long long window;
  int sp, row0, nchunks, pad;
};

struct PairWinArgs {
  const uint8_t* codes;
  const PairWinJob* jobs;  // of this launch
  long long row_stride;
  int n, ngroups;
  unsigned long long* partial;
  unsigned long long* diff;  // [windows][pairs], any may be null
  unsigned long long* both;
  double* dvalue;
};

// pair (i, j), i < j < n, of window w -> index into the outputs
__device__ __forceinline__ long long pmx_win_pair(long long w, long long n, long long i, long long j) {
  return w * (n * (n - 1) / 2) + i * n - i * (i + 1) / 2 + (j - i - 1);
}

// The workgroup's folded sums -> the job's partial row (slot >= 0) or, for a window's only job, the window's results.
// Scan: the PmxScan of the kernel (which tiles exist); red: the folded sums, behind a barrier.
template <class Scan>
__device__ __forceinline__ void pmx_win_store(const PairWinArgs& a, const PairWinJob& job, int R, int C,
                                              const unsigned long long* red, int tid) {
  if (job.slot >= 0) {
    unsigned long long* row = a.partial + (size_t)job.slot * kPmxJobElems;
    for (int k = tid; k < kPmxJobElems; k += kPmxThreads)
      if (Scan::tile_used(k)) row[k] = red[k];
  } else {
    // the window's results: 16 consecutive threads write 16 consecutive pairs (one row of a tile)
    for (int k = tid; k < kPmxJobElems; k += kPmxThreads) {
      if (!Scan::tile_used(k)) continue;
      const int bi = k >> 10, bj = (k >> 8) & 3;
      const long long i = 64ll * R + 16 * bi + ((k >> 4) & 15), j = 64ll * C + 16 * bj + (k & 15);
      if (i < j && j < a.n) {
        const unsigned long long v = red[k], d = v & 0xffffffffull, cc = v >> 32;
        const long long p = pmx_win_pair(job.window, a.n, i, j);
        if (a.diff) a.diff[p] = d;
        if (a.both) a.both[p] = cc;
        if (a.dvalue) a.dvalue[p] = (double)d / (2.0 * (double)cc);
      }
    }
  }
}

template <int NB, bool DIAG, bool AL4>
__global__ __launch_bounds__(kPmxThreads, DIAG ? 2 : 1) void abn_pairwise_win_kernel(const PairWinArgs a) {
  using Scan = PmxScan<NB, DIAG, AL4>;
  constexpr int NF = Scan::NF;
  __shared__ unsigned long long red[kPmxJobElems];
  Scan sc(a.codes);
  const PairWinJob job = a.jobs[blockIdx.x];
  int R, C;
  if constexpr (DIAG) R = C = job.sp;
  else pmx_offdiag(job.sp, a.ngroups, R, C);
#pragma unroll
  for (int b = 0; b < NF; ++b) {
    const int blk = b < 4 ? 4 * R + b : 4 * C + (b - 4);
    int s = 16 * blk + sc.r;
    s = s < a.n ? s : a.n - 1;  // rows past n give sums nobody reads
    sc.roff[b] = (size_t)s * (size_t)a.row_stride + (size_t)job.begin;
  }

  // steps [0, nk_inner): wholly inside the job AND loadable (the row goes on for the loader's spare dword);
  // steps [nk_inner, nk_all): the ragged back, of which those below nk_load are still loadable
  const long long L = job.end - job.begin;
  const long long nk_all = (L + 63) / 64;
  const long long room = a.row_stride - job.begin - (AL4 ? 0 : 4);
  const long long nk_load = room > 0 ? room / 64 : 0;
  const long long nk_inner = L / 64 < nk_load ? L / 64 : nk_load;
  sc.inner_steps(0, nk_inner, red);
  if (sc.wave == kPmxWaves - 1 && nk_inner < nk_all) {
    pmx_u32x4* stage = sc.stage_of(red);
    for (long long k = nk_inner; k < nk_all; ++k) {
      const bool loadable = k < nk_load;  // uniform in the workgroup
      sc.edge_step(k, stage, [&](size_t row_off, long long k0) {
        if (!loadable) return pmx_load_edge(a.codes, row_off, k0, L);
        pmx_u32x4 x = pmx_load<AL4>(a.codes, row_off + (size_t)k0);
#pragma unroll
        for (int d = 0; d < 4; ++d) {  // the sites of the job from dword d of the fragment on: L - k0 - 4 d
          const long long m = L - k0 - 4 * d;
          const uint32_t keep = m >= 4 ? 0xffffffffu : (m <= 0 ? 0u : (1u << (8 * (int)m)) - 1u);
          x[d] = (x[d] & keep) | (0x80808080u & ~keep);
        }
        return x;
      });
    }
    sc.clear_stage(stage);
  }

  __syncthreads();
  sc.fold(red);
  __syncthreads();
  pmx_win_store<Scan>(a, job, R, C, red, sc.tid);
}

// The partial rows of the chunked windows -> their results: pmx_reduce_row per (task, tile, tile row), as
// abn_pairwise_reduce_tiles_kernel does per super-pair of a launch.
__global__ __launch_bounds__(16 * kPmxReduceGroups) void abn_pairwise_win_reduce_kernel(
    const unsigned long long* partial, const PairWinTask* tasks, int n, int ngroups, int diag, unsigned long long* diff,
    unsigned long long* both, double* dvalue) {
  const long long wg = blockIdx.x;
  const PairWinTask t = tasks[wg >> 8];
  const long long base = t.window * ((long long)n * (n - 1) / 2);
  pmx_reduce_row(partial + (size_t)t.row0 * kPmxJobElems, t.nchunks, n, ngroups, diag, t.sp, (int)((wg >> 4) & 15),
                 (int)(wg & 15), diff ? diff + base : nullptr, both ? both + base : nullptr,
                 dvalue ? dvalue + base : nullptr);
}

}  // namespace abn
