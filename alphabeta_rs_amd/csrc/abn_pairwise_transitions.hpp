// The 3 x 3 state transitions of every sample pair — the joint table behind DMatrix::from (src/pedigree.rs:236-257):
//     T[x][y] = #{sites both samples keep : s_a = x, s_b = y},   x, y in {0 = U, 1 = I, 2 = M},  a < b
// on 2-bit packed codes (include/abneutral.h, abn_pack_codes).  The reference keeps two folds of it, both = sum T and
// diff = sum |x - y| T; the table itself is the observed gain / loss spectrum (U -> M, M -> U, the intermediate state).
//
// Plane algebra.  Per sample three 0 / 1 byte planes, looked up from the 2-bit field with v_perm_b32 as pmx_lookup does:
//     u = [field = 0],  i = [field = 1],  m = [field = 2];   field 3 (filtered, padding, masked window edges): 0, 0, 0
// Then T[x][y]_ab = sum_k X_a[k] Y_b[k]: NINE products X_A Y_B^T of a row block A and a column block B on
// v_mfma_i32_16x16x64_i8, 32-bit sums, exact and independent of the order.  Unlike V V^T the products are not symmetric:
// (U I^T)_ab is T[U][I] of the ORDERED pair (a, b) and its transpose belongs to (b, a).  Here the row block is always the
// first operand and never lies behind the column block (R <= C; in a diagonal super-pair bi <= bj), and of a tile on the
// diagonal of a 16-block only the elements row < column are written: x is the state of the lower-numbered sample on
// every kind of tile, with no transposed tile anywhere.
//
// Geometry.  Nine sums per 16 x 16 tile are 36 accumulator registers; the divergence scan's 16 tiles per wavefront would
// be 576, more than the 512 a lane has.  So a job of this scan is one ROW BLOCK of a super-pair: (window, super-pair,
// site chunk, bi) with the tiles (bi, bj) of the 4 column blocks (diagonal super-pairs: bj >= bi, skipped by a scalar
// branch) — 4 tiles x 9 sums x 4 = 144 accumulator registers, 5 fragments per K step (the row block's and the four
// column blocks'), a third of a lane's registers left to the two batches in flight and the planes.  One workgroup per
// CU (__launch_bounds__(256, 1): the whole register file of a SIMD is one wavefront's).  Everything else is PmxScan's:
// the four wavefronts take the batches round-robin with one batch ahead and no LDS tile, the window edges are masked to
// field 3 in registers (PmxPackedWindowFix), the workgroup folds in LDS (32-bit counts, [tile][row][column][9]) and writes
// the window's table itself or, for a chunked window, its quarter of a partial row ([16 tiles][256][9] 32-bit counts; a
// chunk is below 2^30 sites) that abn_pairwise_trans_reduce_kernel sums into 64-bit counts.  No global atomics.  The
// whole matrix is the one window [0, n_sites).  Splitting by row block rather than giving each wavefront its own tiles
// keeps the diagonal super-pairs (n <= 64: the only ones) balanced: their row blocks have 4, 3, 2 and 1 tiles, which as
// jobs of different length spread over the CUs, while as wavefronts of one workgroup they would wait for the longest.
#pragma once
#include <stdint.h>

#include "abn_packed_mask.hpp"

namespace abn {

// The serial host form of the same arithmetic (the CPU tests hold it against an independent model through
// abh_transitions_packed): the table of every pair a < b over the sites [begin, end) of rows of `stride` bytes,
// table[p][3 x + y] in the reference's pair order.
inline unsigned abn_packed_field(const uint8_t* row, long long site) {
  const long long g = site >> 4;
  const int k = (int)(site & 15), j = k >> 2, e = k & 3;  // site 16 g + 4 j + e: byte e of dword g, bits 2j..2j+1
  return (row[4 * g + e] >> (2 * j)) & 3u;
}
inline void abn_transitions_packed_host(const uint8_t* packed, int n, long long stride, long long begin, long long end,
                                        uint64_t* table) {
  long long p = 0;
  for (int a = 0; a < n; ++a)
    for (int b = a + 1; b < n; ++b, ++p) {
      uint64_t* t = table + 9 * p;
      for (int e = 0; e < 9; ++e) t[e] = 0;
      const uint8_t *ra = packed + (size_t)a * (size_t)stride, *rb = packed + (size_t)b * (size_t)stride;
      for (long long k = begin; k < end; ++k) {
        const unsigned x = abn_packed_field(ra, k), y = abn_packed_field(rb, k);
        if (x < 3 && y < 3) ++t[3 * x + y];
      }
    }
}

constexpr int kTransEntries = 9;
constexpr int kTransTileWords = 256 * kTransEntries;   // 32-bit counts of one tile
constexpr int kTransRowWords = 16 * kTransTileWords;   // ... of one partial row: the 4 x 4 tiles of a (super-pair, chunk)
// (super-pair, chunk) units per launch: each is up to four workgroups and, in a chunked window, one 144 KiB partial row
constexpr long long kTransMaxJobs = 2048;

}  // namespace abn

#if defined(__HIPCC__) && defined(ABN_TRANSITIONS_KERNELS)  // (abn_pairwise.hip defines it)
#include "abn_pairwise_windows_packed.hpp"

namespace abn {

// one dword of each 0 / 1 plane from four table indices (pmx_lookup's selector rule; entry 3 is zero in all three)
__device__ __forceinline__ void pmx_trans_lookup(uint32_t y, int& u, int& i, int& m) {
  u = (int)__builtin_amdgcn_perm(0u, 0x00000001u, y);
  i = (int)__builtin_amdgcn_perm(0u, 0x00000100u, y);
  m = (int)__builtin_amdgcn_perm(0u, 0x00010000u, y);
}

// The nine sums of the tiles (bi, bj) of one row block.  Fragment 0 is the row block's, fragment 1 + bj column block bj's.
template <int NB, bool DIAG>
struct PmxTransSums {
  static constexpr int NC = DIAG ? NB : 4;  // column blocks
  static constexpr int NF = NC + 1;
  static constexpr int kRedWords = NC * kTransTileWords / 2;  // 64-bit words of the workgroup's 32-bit counts
  // Between two groups: one step per batch — a second step's fragments in each of the three register sets took that
  // kernel to scratch memory.  Inside a group the batch depth is the divergence scan's: the loads in flight bound it.
  static constexpr int kBatchSteps = DIAG ? pmx_steps(NF) : 1;
  pmx_i32x4 T[NC][kTransEntries];
  int bi;  // the job's row block (uniform in the workgroup)

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < NC; ++j)
#pragma unroll
      for (int k = 0; k < kTransEntries; ++k) T[j][k] = pmx_i32x4{0, 0, 0, 0};
  }
  __device__ __forceinline__ bool tile(int bj) const { return !DIAG || bj >= bi; }
  template <class Codes>
  __device__ __forceinline__ void step(const pmx_u32x4 (&x)[NF], int sub) {
    pmx_i32x4 P[NF][3];  // the planes u, i, m of every fragment
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int u, i, m;
        pmx_trans_lookup(Codes::index(x[f][e], sub), u, i, m);
        P[f][0][e] = u;
        P[f][1][e] = i;
        P[f][2][e] = m;
      }
    // D[row][col] = sum_k A[row][k] B[k][col]: A = plane X of the row block, B = plane Y of the column block — T[X][Y]
    // with X the state of the row sample.  The nine sums of a tile are independent: no dependent pair back to back.
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (tile(j)) {
#pragma unroll
        for (int X = 0; X < 3; ++X)
#pragma unroll
          for (int Y = 0; Y < 3; ++Y)
            T[j][3 * X + Y] = __builtin_amdgcn_mfma_i32_16x16x64_i8(P[0][X], P[1 + j][Y], T[j][3 * X + Y], 0, 0, 0);
      }
  }
  // -> red[column block][row][column][entry], 32-bit counts (C/D layout: column = r, row = 4 q + register)
  __device__ __forceinline__ void fold(unsigned long long* red64, int q, int r) const {
    unsigned* red = reinterpret_cast<unsigned*>(red64);
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (tile(j)) {
#pragma unroll
        for (int k = 0; k < kTransEntries; ++k)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const unsigned v = (unsigned)T[j][k][e];
            if (v) atomicAdd(&red[(j * 256 + (4 * q + e) * 16 + r) * kTransEntries + k], v);
          }
      }
  }
};

struct PairTransArgs {
  const uint8_t* codes;    // the packed rows
  const PairWinJob* jobs;  // of this launch: one per (window, super-pair, chunk); the grid has a workgroup per row block of each
  long long row_stride;    // bytes per row (a multiple of 64 from a 16-byte aligned base)
  int n, ngroups;
  unsigned* partial;             // [rows][kTransRowWords]
  unsigned long long* table;     // [windows][pairs][9]
};

template <int NB, bool DIAG>
__global__ __launch_bounds__(kPmxThreads, 1) void abn_pairwise_trans_kernel(const PairTransArgs a) {
  using Scan = PmxScan<NB, DIAG, true, PmxPackedCodes, PmxTransSums>;
  using Sums = PmxTransSums<NB, DIAG>;
  constexpr int NR = DIAG ? NB : 4;  // row blocks: workgroups per job
  __shared__ unsigned long long red[Sums::kRedWords];
  Scan sc(a.codes);
  sc.wave = __builtin_amdgcn_readfirstlane(sc.wave);
  const PairWinJob job = a.jobs[blockIdx.x / NR];
  const int bi = (int)(blockIdx.x % NR);
  sc.sums.bi = bi;
  int R, C;
  if constexpr (DIAG) R = C = job.sp;
  else pmx_offdiag(job.sp, a.ngroups, R, C);
#pragma unroll
  for (int f = 0; f < Scan::NF; ++f) {
    // (a column block whose tile is skipped reads the row block's bytes again: nothing new from memory)
    const int blk = (f == 0 || !sc.sums.tile(f - 1)) ? 4 * R + bi : 4 * C + (f - 1);
    int s = 16 * blk + sc.r;
    s = s < a.n ? s : a.n - 1;  // rows past n give sums nobody reads
    sc.roff[f] = (size_t)s * (size_t)a.row_stride;
  }

  PmxPackedWindowFix<Scan> mask_edges{job.begin, job.end, sc.q};
  sc.inner_steps(mask_edges.s0(), mask_edges.s1(), red, mask_edges);

  __syncthreads();
  sc.fold(red);
  __syncthreads();
  const unsigned* cnt = reinterpret_cast<const unsigned*>(red);
  if (job.slot >= 0) {
    unsigned* row = a.partial + (size_t)job.slot * kTransRowWords + (size_t)(4 * bi) * kTransTileWords;
    for (int k = sc.tid; k < Sums::NC * kTransTileWords; k += kPmxThreads)
      if (sc.sums.tile(k / kTransTileWords)) row[k] = cnt[k];
  } else {
    // the window's table: consecutive threads write the nine counts of consecutive pairs (one row of a tile: 144 words)
    for (int k = sc.tid; k < Sums::NC * kTransTileWords; k += kPmxThreads) {
      const int bj = k / kTransTileWords, el = (k % kTransTileWords) / kTransEntries, e = k % kTransEntries;
      if (!sc.sums.tile(bj)) continue;
      const long long i = 64ll * R + 16 * bi + (el >> 4), j = 64ll * C + 16 * bj + (el & 15);
      if (i < j && j < a.n) a.table[pmx_win_pair(job.window, a.n, i, j) * kTransEntries + e] = cnt[k];
    }
  }
}

// The partial rows of the chunked windows -> their tables.  A workgroup owns one row of one tile of one (window,
// super-pair): 144 consecutive counts per partial row; four thread groups take the chunks in turn, LDS combines them.
constexpr int kTransReduceGroups = 4;
constexpr int kTransReduceRow = 16 * kTransEntries;
__global__ __launch_bounds__(kTransReduceRow* kTransReduceGroups) void abn_pairwise_trans_reduce_kernel(
    const unsigned* partial, const PairWinTask* tasks, int n, int ngroups, int diag, unsigned long long* table) {
  __shared__ unsigned long long acc[kTransReduceGroups][kTransReduceRow];
  const long long wg = blockIdx.x;
  const PairWinTask t = tasks[wg >> 8];
  const int tile = (int)((wg >> 4) & 15), trow = (int)(wg & 15);
  int R, C;
  if (diag) R = C = t.sp;
  else pmx_offdiag(t.sp, ngroups, R, C);
  const int bi = tile >> 2, bj = tile & 3;
  const long long i = 64ll * R + 16 * bi + trow, j0 = 64ll * C + 16 * bj;
  // the whole workgroup leaves together when its row holds no pair (that covers the tiles no job writes: bj < bi of a
  // diagonal super-pair, blocks past n)
  if (i >= n || j0 >= n || j0 + 15 <= i) return;
  const int v = threadIdx.x % kTransReduceRow, grp = threadIdx.x / kTransReduceRow;
  const unsigned* src = partial + (size_t)t.row0 * kTransRowWords + tile * kTransTileWords + trow * kTransReduceRow + v;
  unsigned long long s = 0;
#pragma unroll 4
  for (int c = grp; c < t.nchunks; c += kTransReduceGroups) s += src[(size_t)c * kTransRowWords];
  acc[grp][v] = s;
  __syncthreads();
  if (grp == 0) {
    for (int g = 1; g < kTransReduceGroups; ++g) s += acc[g][v];
    const long long j = j0 + v / kTransEntries;
    if (i < j && j < n) table[pmx_win_pair(t.window, n, i, j) * kTransEntries + v % kTransEntries] = s;
  }
}

}  // namespace abn
#endif  // kernels
