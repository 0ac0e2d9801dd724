// Pairwise divergence on 2-bit packed codes — DMatrix::from (src/pedigree.rs:210-261): a packed front end of the Gram
// product scan of abn_pairwise_mx.hpp.  Same job geometry, same register pipeline, LDS fold, partial rows, reduce
// kernel and pair order (PmxScan, abn_pairwise_reduce_tiles_kernel); what differs is what a loaded dword holds.
//
// Format (include/abneutral.h, abn_pack_codes): one 2-bit field per (sample, site), 0 = U, 1 = I, 2 = M (status_numeric,
// src/methylation_site.rs:130-136), 3 = filtered for this sample (src/pedigree.rs:249-251).  Sites in groups of 16, one
// little-endian dword p per group: site 16 g + 4 j + e sits in byte e of dword g at bits 2j..2j+1, so that
//     (p >> 2j) & 0x03030303,  j = 0..3
// is a dword of four byte-sized table indices — ready for the three v_perm_b32 plane look-ups of pmx_lookup, whose
// entry 3 is v = i = z = 0.  A shift-and-mask and three permutes per four sites and sample: what the byte path spends
// (pmx_planes).  Which site lands in which k slot of a matrix step does not matter: both operands of A A^T use the same
// assignment and the sums are integers (the header of abn_pairwise_mx.hpp relies on the same).
//
// The 16 bytes lane l loads from row (l & 15) of a 16-sample block at byte offset 64 s + 16 (l >> 4) of "super-step" s
// hold 64 sites of that sample — four dwords x four shifts: the lane's operand fragments of FOUR K = 64 matrix steps,
// where a fragment of byte codes feeds one.  A wavefront so consumes a row at a quarter of the byte scan's load rate for
// the same matrix work.  The loaders deal in 64-byte steps of a row whatever they hold, so the batch depth in super-steps
// is pmx_steps(NF) as in the byte kernel: the bytes a lane keeps in flight stay at kPmxFrags fragments per batch, the
// matrix steps per batch are four times the byte kernel's.
//
// Rows start at multiples of 64 bytes (256 sites) from a 16-byte aligned base and every field from site L to the end
// of the row is 3 (filtered): no ragged-edge loader, no unaligned loader, no AL4 variants.  The kernel reads the first
// ceil(L / 256) super-steps of every row and nothing behind them.  (Many column ranges of one packed matrix in one
// call: abn_pairwise_windows_packed.hpp.)
#pragma once
#include "abn_pairwise_mx.hpp"

namespace abn {

struct PmxPackedCodes {
  static constexpr int SUB = 4;  // K steps a fragment feeds: one per shift
  // the four table indices of shift j of a dword
  static __device__ __forceinline__ uint32_t index(uint32_t p, int j) { return (p >> (2 * j)) & 0x03030303u; }
  static __device__ __forceinline__ void planes(uint32_t p, int j, int& v, int& i, int& z) {
    pmx_lookup(index(p, j), v, i, z);
  }
};

struct PairPackedArgs {
  const uint8_t* packed;
  long long row_stride;  // bytes per sample: a multiple of 64
  long long nk;          // super-steps (64 bytes = 256 sites) of a row that hold sites: ceil(L / 256) <= row_stride / 64
  int n;                 // samples
  int ngroups;           // groups of 64 samples
  int nchunks;           // chunks of super-steps per super-pair
  long long first;       // this launch's first super-pair, as PairMxArgs::first
  unsigned long long* partial;  // [super-pairs of the launch * nchunks][16 tiles][256]
};

template <int NB, bool DIAG>
__global__ __launch_bounds__(kPmxThreads, DIAG ? 2 : 1) void abn_pairwise_packed_kernel(const PairPackedArgs a) {
  using Scan = PmxScan<NB, DIAG, true, PmxPackedCodes>;
  __shared__ unsigned long long red[kPmxJobElems];
  Scan sc(a.packed);
  // job -> (super-pair, chunk)
  const long long job = blockIdx.x;
  const int chunk = (int)(job % a.nchunks);
  const long long spl = job / a.nchunks;  // super-pair of the launch
  int R, C;
  if constexpr (DIAG) R = C = (int)(a.first + spl);
  else pmx_offdiag(a.first + spl, a.ngroups, R, C);

  // this lane's byte offset in each block's row: sample (clamped: rows past n give sums nobody reads) x stride
#pragma unroll
  for (int b = 0; b < Scan::NF; ++b) {
    const int blk = b < 4 ? 4 * R + b : 4 * C + (b - 4);
    int s = 16 * blk + sc.r;
    s = s < a.n ? s : a.n - 1;
    sc.roff[b] = (size_t)s * (size_t)a.row_stride;
  }

  // The super-steps are split evenly over the super-pair's chunks, at multiples of two (whole 128-byte lines of a row, as
  // in the byte kernel).  Every one of them lies inside every row: the padding is part of the format.
  const long long nk2 = a.nk / 2;
  const long long Ks = 2 * ((long long)chunk * nk2 / a.nchunks);
  const long long Ke = chunk == a.nchunks - 1 ? a.nk : 2 * ((long long)(chunk + 1) * nk2 / a.nchunks);
  sc.inner_steps(Ks, Ke, red);

  // ---- the workgroup's sums
  __syncthreads();
  sc.fold(red);
  __syncthreads();
  unsigned long long* row = a.partial + (spl * a.nchunks + chunk) * kPmxJobElems;
  for (int k = sc.tid; k < kPmxJobElems; k += kPmxThreads)
    if (Scan::tile_used(k)) row[k] = red[k];
}

}  // namespace abn
