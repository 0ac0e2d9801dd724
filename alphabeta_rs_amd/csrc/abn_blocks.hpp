// Block bootstrap over genomic blocks (abn_block_*, abn_tiles_block_bootstrap): the uncertainty of a rate estimated for a
// pool of regions or for a genome cut into tiles.  The reference's residual bootstrap (src/boot_model.rs:43-57) resamples
// the N rows of one pedigree and keeps the observed site counts; here the BLOCKS — the merged segments of a pool, the
// fixed tiles of a genome — are drawn with replacement, and every pair's diff and both (src/pedigree.rs:236-257) and every
// sample's level fold (src/pedigree.rs:159-172) are formed again from the drawn blocks.
//
// T blocks in G groups; group g owns the contiguous ascending block range [gb_g, ge_g), T_g = ge_g - gb_g.  Every group
// has R + 1 ROWS of counts: rows 0 .. R - 1 are drawn replicates, row R is the identity row (every count 1: the observed
// data through the same kernels).  A row's count c[t] says how often block t was drawn; a delete-one-block jackknife is
// a row of ones with one zero (abn_block_resample takes any counts).
//
//   counts   row r of group g makes T_g draws; draw j is block gb_g + index_from(word, T_g), word = element j % 4 of
//            philox4x32_10(j / 4, r, group_id[g], kTagBlock, seed_lo, seed_hi) — the counter layout of abn_gen_idx_kernel,
//            so a row depends on neither R nor G.  c[row][t] is the histogram of the draws, a byte.  A workgroup keeps
//            kBlockHist 32-bit bins in LDS (integer LDS atomics: the sum does not depend on their order); a group of more
//            blocks is cut into chunks of kBlockHist bins, and every chunk's workgroup walks all T_g draws and counts those
//            that fall into its chunk (the second path: ceil(T_g / kBlockHist) times the draws).  A count above
//            kBlockCountMax raises a flag and the entry fails; it is never clamped.
//   digits   every table value v < 2^35 is split into 7-bit digits v = sum_d digit_d 2^(7 d), signed bytes 0 .. 127;
//            D = max(1, ceil(bitlen / 7)) of the largest value of both tables (diff <= 2 both in a scan's tables, so this
//            is the bit length of 2 both there; explicit tables may hold anything below 2^35).  Plane (table, d) is a
//            byte matrix [column][block], blocks padded to a multiple of 64 and columns to one of 16 with zeros: the
//            B operand of v_mfma_i32_16x16x64_i8 — lane l holds B[k = 16 (l >> 4) + j][column l & 15] in byte j, 16
//            consecutive blocks of one column, one aligned 16-byte load.
//   product  D[row][column] = sum_k c[row][k] digit[k][column] on v_mfma_i32_16x16x64_i8.  A = the counts: lane l holds
//            c[row l & 15][k = 16 (l >> 4) + j] in byte j.  (Both operands use the same k of byte j of lane group l >> 4,
//            so the sum over k is the same whatever order the instruction gives the 64 k.)  A job is (group, kBlockRowTiles
//            16-row tiles, 16-column tile): one wavefront, K over the group's blocks alone in steps of 64 aligned to
//            multiples of 64, the two edge steps masked byte by byte (a group begins and ends at any block).  A product
//            is at most 127 x 127; the 32-bit sums are flushed into 64-bit ones every kBlockFlush blocks (127^2 x 131072 <
//            2^31) and the digits recombined by shifts: both*[row][p] = sum_t c[row][t] both[t][p], diff* likewise,
//            exact.  C/D layout: column = l & 15, row = 4 (l >> 4) + register.  No global atomics, no scratch.
//   finish   dvalue* = (double)diff* / (2.0 * (double)both*), the expression of src/pedigree.rs:257 (0 / 0 stays NaN).
//   levels   a lane per (row, sample): level*[row][s] = sum_t (double)c level_sum_kept[s][t], serial in ascending t within
//            the group from +0.0, every term a rounded product and a rounded add (no fma); kept* = sum_t c kept[s][t], exact.
//            The two tables are transposed to [T][n] first: neighbouring lanes differ in the sample and read neighbours.
//
// Limits (block_shape_refusal, block_tables_refusal, block_counts_refusal; host only, before any launch): a table value >=
// 2^35, more than 2^21 blocks in a group (127 x 2^35 x 2^21 <= 2^63: every sum stays below 2^63), R > 2^20 - 2, G > 4096,
// null pointers, negative sizes, unordered or overlapping group ranges, a count above 127.  Tables and counts that live on
// the device (abn_block_resample_dev, abn_tiles_block_bootstrap) the host has not seen: there the kernels find a value of
// 2^35 or a count of 128 themselves, the entry fails AFTER the run, and what it wrote to the outputs is no result.  An
// empty group is no error: its sums are 0, its dvalue NaN.
//
// The arithmetic and the serial forms compile without a HIP header (tests/native/blocks_main.cpp includes this file).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "abn_philox.h"

namespace abn {

constexpr int kBlockCountMax = 127;                        // a count is a signed byte 0 .. 127
constexpr int kBlockDigitBits = 7;
constexpr long long kBlockValueEnd = 1LL << 35;            // table values lie below
constexpr int kBlockDigitsMax = 5;                         // ceil(35 / 7)
constexpr long long kBlockFlush = 131072;                  // blocks between two flushes of the 32-bit sums, at the most
constexpr int kBlockHist = 8192;                           // the bins of one workgroup's histogram (32 KiB of LDS)
constexpr long long kBlockGroupMax = 1LL << 21;            // blocks in a group
constexpr long long kBlockReplicatesMax = (1LL << 20) - 2; // R: row ids 0 .. 2^20 - 2, the identity row's is 2^20 - 1
constexpr int kBlockGroupsMax = 4096;
constexpr int kBlockRowTiles = 2;                          // 16-row tiles of one product job
constexpr int kBlockThreads = 256;
static_assert(127LL * 127 * kBlockFlush < (1LL << 31), "the 32-bit sums between two flushes");
static_assert(kBlockFlush % 64 == 0, "a flush falls between two K steps");
static_assert(kBlockDigitsMax * kBlockDigitBits >= 35, "digits of a table value");

// draw j of a row from the four words of counter j / 4
ABN_HD void block_draw_words(uint64_t seed, uint32_t group_id, uint32_t row, uint32_t quad, uint32_t out[4]) {
  philox4x32_10(quad, row, group_id, kTagBlock, (uint32_t)seed, (uint32_t)(seed >> 32), out);
}
ABN_HD int block_digits_of(uint64_t largest) {
  int bits = 0;
  while (largest) ++bits, largest >>= 1;
  const int d = (bits + kBlockDigitBits - 1) / kBlockDigitBits;
  return d < 1 ? 1 : d;
}
ABN_HD uint32_t block_digit(uint64_t v, int d) { return (uint32_t)(v >> (kBlockDigitBits * d)) & 127u; }
ABN_HD double block_dvalue(uint64_t diff, uint64_t both) { return (double)diff / (2.0 * (double)both); }
// one term of a level sum: a rounded product, then a rounded add
ABN_HD double block_level_step(double acc, uint32_t count, double level) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double term = (double)count * level;
  return acc + term;
}

// ---- the argument checks, host only: an empty text takes the arguments
inline std::string block_shape_refusal(long long n_groups, const int64_t* group_begin, const int64_t* group_end,
                                       long long rows_per_group, long long n_blocks) {
  if (n_groups < 0 || rows_per_group < 0 || n_blocks < 0) return "a negative size";
  if (n_groups > kBlockGroupsMax) return "more than 4096 groups";
  if (rows_per_group - 1 > kBlockReplicatesMax) return "more than 2^20 - 2 replicates";
  if (n_groups > 0 && (!group_begin || !group_end)) return "null/size";
  long long last = 0;
  for (long long g = 0; g < n_groups; ++g) {
    const long long b = group_begin[g], e = group_end[g];
    if (b < last || e < b || e > n_blocks)
      return "group " + std::to_string(g) + ": its block range [" + std::to_string(b) + ", " + std::to_string(e) +
             ") is unordered, overlaps the group in front of it or leaves the " + std::to_string(n_blocks) + " blocks";
    if (e - b > kBlockGroupMax) return "group " + std::to_string(g) + ": more than 2^21 blocks";
    last = e;
  }
  return "";
}
inline std::string block_tables_refusal(long long n_blocks, long long n_pairs, long long n_samples, const uint64_t* both,
                                        const uint64_t* diff, const double* level_sum_kept, const int64_t* kept,
                                        uint64_t* largest) {
  if (n_pairs < 0 || n_samples < 0) return "a negative size";
  if (n_blocks > 0 && ((n_pairs > 0 && (!both || !diff)) || (n_samples > 0 && (!level_sum_kept || !kept))))
    return "null/size";
  uint64_t any = 0;
  for (long long i = 0; i < n_blocks * n_pairs; ++i) any |= both[i] | diff[i];
  if (any >= (uint64_t)kBlockValueEnd) return "a table value of 2^35 or more";
  if (largest) *largest = any;  // (its bit length is the largest value's)
  return "";
}
// the counts inside the groups' ranges: the first above 127, as a text
inline std::string block_counts_refusal(long long n_groups, const int64_t* group_begin, const int64_t* group_end,
                                        long long rows_per_group, long long n_blocks, const uint8_t* counts) {
  if (n_groups > 0 && rows_per_group > 0 && n_blocks > 0 && !counts) return "null/size";
  for (long long g = 0; g < n_groups; ++g)
    for (long long r = 0; r < rows_per_group; ++r) {
      const uint8_t* c = counts + (size_t)(g * rows_per_group + r) * (size_t)n_blocks;
      for (long long t = group_begin[g]; t < group_end[g]; ++t)
        if (c[t] > kBlockCountMax)
          return "group " + std::to_string(g) + ", row " + std::to_string(r) + ", block " + std::to_string(t) + ": a count of " +
                 std::to_string((int)c[t]) + ", above 127";
    }
  return "";
}

// ---- the serial forms
// counts [G x (R + 1) x T], zero outside a group's range; false: a count above 127 (the bytes are then no result)
inline bool block_counts_host(uint64_t seed, long long n_groups, const uint32_t* group_id, const int64_t* group_begin,
                              const int64_t* group_end, long long n_replicates, long long n_blocks, uint8_t* counts) {
  bool ok = true;
  std::vector<uint32_t> hist;
  const long long rows = n_replicates + 1;
  for (long long g = 0; g < n_groups; ++g) {
    const long long b = group_begin[g], Tg = group_end[g] - b;
    for (long long r = 0; r < rows; ++r) {
      uint8_t* c = counts + (size_t)(g * rows + r) * (size_t)n_blocks;
      for (long long t = 0; t < n_blocks; ++t) c[t] = 0;
      if (r == n_replicates) {
        for (long long t = 0; t < Tg; ++t) c[b + t] = 1;
        continue;
      }
      hist.assign((size_t)Tg, 0u);
      for (long long q = 0; 4 * q < Tg; ++q) {
        uint32_t w[4];
        block_draw_words(seed, group_id[g], (uint32_t)r, (uint32_t)q, w);
        for (int e = 0; e < 4 && 4 * q + e < Tg; ++e) ++hist[index_from(w[e], (uint32_t)Tg)];
      }
      for (long long t = 0; t < Tg; ++t) {
        if (hist[(size_t)t] > (uint32_t)kBlockCountMax) ok = false;
        c[b + t] = (uint8_t)hist[(size_t)t];
      }
    }
  }
  return ok;
}

// the sums of every row: both_out, diff_out, dvalue_out [G x rows x P], level_out, kept_out [G x rows x n]; any may be null
inline void block_resample_host(long long n_groups, const int64_t* group_begin, const int64_t* group_end,
                                long long rows_per_group, const uint8_t* counts, long long n_blocks, long long n_pairs,
                                long long n_samples, const uint64_t* both, const uint64_t* diff, const double* level_sum_kept,
                                const int64_t* kept, uint64_t* both_out, uint64_t* diff_out, double* dvalue_out,
                                double* level_out, int64_t* kept_out) {
  const size_t P = (size_t)n_pairs;
  std::vector<uint64_t> sb(P), sd(P);
  for (long long g = 0; g < n_groups; ++g)
    for (long long r = 0; r < rows_per_group; ++r) {
      const size_t row = (size_t)(g * rows_per_group + r);
      const uint8_t* c = counts + row * (size_t)n_blocks;
      if (P > 0 && (both_out || diff_out || dvalue_out)) {
        std::fill(sb.begin(), sb.end(), 0), std::fill(sd.begin(), sd.end(), 0);
        for (long long t = group_begin[g]; t < group_end[g]; ++t) {
          const uint64_t w = c[t];
          if (!w) continue;
          const uint64_t *tb = both + (size_t)t * P, *td = diff + (size_t)t * P;
          for (size_t p = 0; p < P; ++p) sb[p] += w * tb[p], sd[p] += w * td[p];
        }
        for (size_t p = 0; p < P; ++p) {
          if (both_out) both_out[row * P + p] = sb[p];
          if (diff_out) diff_out[row * P + p] = sd[p];
          if (dvalue_out) dvalue_out[row * P + p] = block_dvalue(sd[p], sb[p]);
        }
      }
      for (long long s = 0; s < n_samples; ++s) {
        double level = 0.0;
        int64_t k = 0;
        for (long long t = group_begin[g]; t < group_end[g]; ++t) {
          level = block_level_step(level, c[t], level_sum_kept[s * n_blocks + t]);
          k += (int64_t)c[t] * kept[s * n_blocks + t];
        }
        if (level_out) level_out[row * (size_t)n_samples + (size_t)s] = level;
        if (kept_out) kept_out[row * (size_t)n_samples + (size_t)s] = k;
      }
    }
}

// blocks padded to whole K steps, columns to whole tiles: the planes' shape
inline long long block_padded_blocks(long long n_blocks) { return (n_blocks + 63) / 64 * 64; }
inline long long block_padded_pairs(long long n_pairs) { return (n_pairs + 15) / 16 * 16; }
// the workgroups of a grid-stride launch over `values` elements
inline unsigned block_grid(long long values) {
  const long long wg = (values + kBlockThreads - 1) / kBlockThreads;
  return (unsigned)(wg < 1 ? 1 : wg > (1 << 20) ? (1 << 20) : wg);
}
constexpr long long kBlockJobsMax = 1LL << 23;  // product jobs of one group: a grid's x extent times 256 lanes stays below 2^32

#if defined(__HIPCC__) && defined(ABN_BLOCKS_KERNELS)  // (abn_blocks.hip defines it)
// ------------------------------------------------------------------------------------------------ kernels
struct BlockMeta {           // what the kernels leave for one another and for the host
  unsigned long long any;    // the OR of every table value: its bit length is the largest value's
  int over_count;            // a count above 127 (the counts kernel, or the product's read of explicit counts)
  int over_value;            // a table value of 2^35 or more (device tables: the host has not seen them)
};

// grid: (R + 1, G, chunks of the largest group); block kBlockThreads.  counts [G x (R + 1) x T] is zero on entry.
__global__ void __launch_bounds__(kBlockThreads)
abn_block_counts_kernel(uint64_t seed, const uint32_t* __restrict__ group_id, const long long* __restrict__ group_begin,
                        const long long* __restrict__ group_end, int n_replicates, long long n_blocks,
                        uint8_t* __restrict__ counts, BlockMeta* __restrict__ meta) {
  __shared__ uint32_t hist[kBlockHist];
  const int row = blockIdx.x, g = blockIdx.y;
  const long long b = group_begin[g], Tg = group_end[g] - b;
  const long long chunk = (long long)blockIdx.z * kBlockHist;  // the bins of this workgroup: [chunk, chunk + bins)
  if (chunk >= Tg) return;
  const int bins = (int)(Tg - chunk < kBlockHist ? Tg - chunk : kBlockHist);
  uint8_t* out = counts + ((size_t)g * (size_t)(n_replicates + 1) + (size_t)row) * (size_t)n_blocks + (size_t)(b + chunk);
  if (row == n_replicates) {  // the identity row
    for (int i = threadIdx.x; i < bins; i += kBlockThreads) out[i] = 1;
    return;
  }
  for (int i = threadIdx.x; i < bins; i += kBlockThreads) hist[i] = 0u;
  __syncthreads();
  const uint32_t gid = group_id[g];
  for (long long q = threadIdx.x; 4 * q < Tg; q += kBlockThreads) {
    uint32_t w[4];
    block_draw_words(seed, gid, (uint32_t)row, (uint32_t)q, w);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long at = (long long)index_from(w[e], (uint32_t)Tg) - chunk;
      if (4 * q + e < Tg && at >= 0 && at < bins) atomicAdd(&hist[at], 1u);
    }
  }
  __syncthreads();
  bool over = false;
  for (int i = threadIdx.x; i < bins; i += kBlockThreads) {
    const uint32_t v = hist[i];
    over |= v > (uint32_t)kBlockCountMax;
    out[i] = (uint8_t)v;
  }
  if (over) meta->over_count = 1;  // (every writer writes the same word)
}

// grid: ceil(values / (kBlockThreads x 8)); the OR of both tables' values into meta->any, one atomic per workgroup
__global__ void __launch_bounds__(kBlockThreads)
abn_block_largest_kernel(const unsigned long long* __restrict__ both, const unsigned long long* __restrict__ diff,
                         long long values, BlockMeta* __restrict__ meta) {
  __shared__ unsigned long long part[kBlockThreads];
  unsigned long long any = 0;
  for (long long i = (long long)blockIdx.x * kBlockThreads + threadIdx.x; i < values; i += (long long)gridDim.x * kBlockThreads)
    any |= both[i] | diff[i];
  part[threadIdx.x] = any;
  __syncthreads();
  for (int d = kBlockThreads / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) part[threadIdx.x] |= part[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0 && part[0]) {
    atomicOr(&meta->any, part[0]);
    if (part[0] >= (unsigned long long)kBlockValueEnd) meta->over_value = 1;
  }
}

__device__ __forceinline__ int block_digits_dev(const BlockMeta* meta, int planes_per_table) {
  const int d = block_digits_of(meta->any);
  return d < planes_per_table ? d : planes_per_table;  // (more only behind over_value: the entry fails)
}

// grid: (Tpad / 64, Ppad / 16); a workgroup turns the 64 blocks x 16 columns of both tables into their bytes of every
// plane: plane (table, d) [Ppad][Tpad] at planes + (table x planes_per_table + d) x Ppad x Tpad; zeros past T and P
__global__ void __launch_bounds__(kBlockThreads)
abn_block_digits_kernel(const unsigned long long* __restrict__ both, const unsigned long long* __restrict__ diff,
                        long long n_blocks, long long n_pairs, long long Tpad, long long Ppad, int planes_per_table,
                        const BlockMeta* __restrict__ meta, uint8_t* __restrict__ planes) {
  __shared__ unsigned long long v[2][64][16 + 1];
  const long long t0 = (long long)blockIdx.x * 64, p0 = (long long)blockIdx.y * 16;
  const int D = block_digits_dev(meta, planes_per_table);
  {  // consecutive lanes, consecutive columns of one block
    const int pp = threadIdx.x & 15;
    for (int tt = threadIdx.x >> 4; tt < 64; tt += kBlockThreads / 16) {
      const long long t = t0 + tt, p = p0 + pp;
      const bool in = t < n_blocks && p < n_pairs;
      v[0][tt][pp] = in ? both[t * n_pairs + p] : 0ull;
      v[1][tt][pp] = in ? diff[t * n_pairs + p] : 0ull;
    }
  }
  __syncthreads();
  // 16 lanes write the 64 bytes of one column: four blocks a lane
  const int pp = threadIdx.x >> 4, t4 = 4 * (threadIdx.x & 15);
  const size_t plane_bytes = (size_t)Ppad * (size_t)Tpad;
  for (int tab = 0; tab < 2; ++tab)
    for (int d = 0; d < D; ++d) {
      uint32_t word = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) word |= block_digit(v[tab][t4 + e][pp], d) << (8 * e);
      uint8_t* dst = planes + (size_t)(tab * planes_per_table + d) * plane_bytes + (size_t)(p0 + pp) * (size_t)Tpad + (size_t)(t0 + t4);
      *reinterpret_cast<uint32_t*>(dst) = word;
    }
}

typedef int blk_i32x4 __attribute__((ext_vector_type(4)));

struct BlockGemmArgs {
  const uint8_t* counts;            // [G x rows x T]
  const uint8_t* planes;            // [2 x planes_per_table][Ppad][Tpad]
  const long long *group_begin, *group_end;
  BlockMeta* meta;
  unsigned long long *both_out, *diff_out;  // [G x rows x P]
  long long n_blocks, n_pairs, Tpad, Ppad;
  int rows, planes_per_table;
  int row_jobs, col_jobs;           // per group: ceil(rows / (16 kBlockRowTiles)), ceil(Ppad / 16 / 4)
};

// grid: (row_jobs x col_jobs, G) workgroups of four wavefronts; wavefront w takes column tile 4 x (column job) + w
__global__ void __launch_bounds__(kBlockThreads)
abn_block_gemm_kernel(const BlockGemmArgs a) {
  constexpr int RT = kBlockRowTiles, DM = kBlockDigitsMax;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int r = lane & 15, q = lane >> 4;
  const int cj = (int)(blockIdx.x % (unsigned)a.col_jobs), rj = (int)(blockIdx.x / (unsigned)a.col_jobs), g = blockIdx.y;
  const long long ct = 4ll * cj + wave;
  if (16 * ct >= a.Ppad) return;  // (wave-uniform: the MFMAs below run with every lane)
  const long long b = a.group_begin[g], e = a.group_end[g];
  const int D = block_digits_dev(a.meta, a.planes_per_table);
  const size_t plane_bytes = (size_t)a.Ppad * (size_t)a.Tpad;
  const uint8_t* bcol = a.planes + (size_t)(16 * ct + r) * (size_t)a.Tpad;
  const uint8_t* arow[RT];
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    long long row = 16ll * (RT * rj + i) + r;
    row = row < a.rows ? row : a.rows - 1;  // rows past the group's give sums nobody writes
    arow[i] = a.counts + ((size_t)g * (size_t)a.rows + (size_t)row) * (size_t)a.n_blocks;
  }
  blk_i32x4 acc[RT][2][DM];
  unsigned long long sum[RT][2][4];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int tab = 0; tab < 2; ++tab) {
#pragma unroll
      for (int d = 0; d < DM; ++d) acc[i][tab][d] = blk_i32x4{0, 0, 0, 0};
#pragma unroll
      for (int x = 0; x < 4; ++x) sum[i][tab][x] = 0ull;
    }
  auto flush = [&]() {
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int tab = 0; tab < 2; ++tab)
#pragma unroll
        for (int d = 0; d < DM; ++d) {
#pragma unroll
          for (int x = 0; x < 4; ++x) sum[i][tab][x] += (unsigned long long)(uint32_t)acc[i][tab][d][x] << (kBlockDigitBits * d);
          acc[i][tab][d] = blk_i32x4{0, 0, 0, 0};
        }
  };
  uint32_t over = 0u;
  int steps = 0;
  for (long long k = b & ~63ll; k < e; k += 64) {
    const long long kk = k + 16 * q;  // this lane's 16 blocks
    const bool inside = kk >= b && kk + 16 <= e;
    blk_i32x4 av[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (inside) {
        __builtin_memcpy(w, arow[i] + kk, 16);  // (inside [b, e), so inside the row; aligned to nothing)
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const long long t = kk + j;
          if (t >= b && t < e) w[j >> 2] |= (uint32_t)arow[i][t] << (8 * (j & 3));
        }
      }
      over |= (w[0] | w[1] | w[2] | w[3]) & 0x80808080u;
      av[i] = blk_i32x4{(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
    }
#pragma unroll
    for (int tab = 0; tab < 2; ++tab)
#pragma unroll
      for (int d = 0; d < DM; ++d)
        if (d < D) {  // (uniform)
          // kk + 16 <= Tpad, and Tpad is a multiple of 64 behind an aligned base: one aligned 16-byte load
          const blk_i32x4 bv = *reinterpret_cast<const blk_i32x4*>(bcol + (size_t)(tab * a.planes_per_table + d) * plane_bytes + (size_t)kk);
#pragma unroll
          for (int i = 0; i < RT; ++i) acc[i][tab][d] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[i], bv, acc[i][tab][d], 0, 0, 0);
        }
    if (++steps == (int)(kBlockFlush / 64)) {
      flush();
      steps = 0;
    }
  }
  flush();
  if (over) a.meta->over_count = 1;  // (every writer writes the same word)
  const long long col = 16 * ct + r;
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const long long row = 16ll * (RT * rj + i) + 4 * q + x;
      if (row < a.rows && col < a.n_pairs) {
        const size_t at = ((size_t)g * (size_t)a.rows + (size_t)row) * (size_t)a.n_pairs + (size_t)col;
        a.both_out[at] = sum[i][0][x];
        a.diff_out[at] = sum[i][1][x];
      }
    }
}

// grid: block_grid(values), grid-stride
__global__ void __launch_bounds__(kBlockThreads)
abn_block_finish_kernel(const unsigned long long* __restrict__ both, const unsigned long long* __restrict__ diff,
                        long long values, double* __restrict__ dvalue) {
  for (long long i = (long long)blockIdx.x * kBlockThreads + threadIdx.x; i < values; i += (long long)gridDim.x * kBlockThreads)
    dvalue[i] = block_dvalue(diff[i], both[i]);
}

// grid: block_grid(n x T), grid-stride; the tables [n][T] -> [T][n], so that the lanes of the levels kernel, which differ in
// the sample, read neighbouring words
__global__ void __launch_bounds__(kBlockThreads)
abn_block_transpose_kernel(const double* __restrict__ level_sum_kept, const long long* __restrict__ kept, long long n_blocks,
                           int n_samples, double* __restrict__ level_by_block, long long* __restrict__ kept_by_block) {
  const long long total = n_blocks * n_samples;
  for (long long i = (long long)blockIdx.x * kBlockThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kBlockThreads) {
    const long long s = i / n_blocks, t = i % n_blocks;
    level_by_block[t * n_samples + s] = level_sum_kept[i];
    kept_by_block[t * n_samples + s] = kept[i];
  }
}

// grid: block_grid(G x rows x n), grid-stride; a lane per (group, row, sample), the sample fastest; the tables by block:
// level_by_block, kept_by_block [T][n] (abn_block_transpose_kernel).  The chain of a lane is the serial host form's.
__global__ void __launch_bounds__(kBlockThreads)
abn_block_levels_kernel(const uint8_t* __restrict__ counts, const long long* __restrict__ group_begin,
                        const long long* __restrict__ group_end, int n_groups, int rows, long long n_blocks, int n_samples,
                        const double* __restrict__ level_by_block, const long long* __restrict__ kept_by_block,
                        double* __restrict__ level_out, long long* __restrict__ kept_out) {
  const long long total = (long long)n_groups * rows * n_samples;
  for (long long i = (long long)blockIdx.x * kBlockThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kBlockThreads) {
    const long long s = i % n_samples, grow = i / n_samples;
    const int g = (int)(grow / rows);
    const uint8_t* c = counts + (size_t)grow * (size_t)n_blocks;
    double level = 0.0;
    long long k = 0;
    for (long long t = group_begin[g]; t < group_end[g]; ++t) {
      const uint32_t w = c[t];
      level = block_level_step(level, w, level_by_block[t * n_samples + s]);
      k += (long long)w * kept_by_block[t * n_samples + s];
    }
    if (level_out) level_out[i] = level;
    if (kept_out) kept_out[i] = k;
  }
}
#endif  // kernels

}  // namespace abn
