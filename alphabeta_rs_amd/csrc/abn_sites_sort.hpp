// One resident methylome's records sorted by genomic position, on the device (abn_sites_sort, abn_sites_sort_keys): a
// stable least-significant-digit radix sort of (key, index) pairs by (chromosome, start, end, strand) — inside a
// chromosome the order of common_key_less (abn_sites_common.hpp), the chromosomes in the order of their keys (0..255,
// M = 256, C = 257), equal keys in file order.
//
// The KEY has 75 significant bits, most significant first chromosome (9), start (32), end (32), strand (2), held in three
// words: w[0] = strand | end << 2, w[1] = end >> 30 | start << 2, w[2] = start >> 30 | chromosome << 2.  A DIGIT is 8
// bits: pass p reads bits 8p .. 8p + 7 of the key, byte p % 4 of word p / 4, so no digit straddles a word; ten passes
// (kSortPasses) read every bit once, the last one the three bits that are left.  A pass whose digit is the same in every
// key — found from the OR and the AND of all keys, which the check kernel reduces — moves nothing and is skipped:
// chromosomes below 256 make pass 9 constant, short sites (end - start small) make the high bytes of `end` follow those
// of `start`, and a file already in order skips all ten.
//
// A pair is one uint4 {w[0], w[1], w[2], index}: 16 B read and 16 B written per pair and pass.  A TILE is kSortTile =
// kSortThreads x kSortItems = 2048 consecutive pairs, one workgroup; lane t of the workgroup holds pairs t, t + 256, ..
// of the tile (coalesced 16-byte loads), so the tile is 32 GROUPS of 64 consecutive pairs, group g = item * 4 + wave.
//
//   abn_sort_flatten_*_kernel  the merge of abn_sites_merge.hpp with an output that keeps the record: meta, start, end,
//                              posteriormax, meth_lvl of every site in file order (search and one-writer structure as there)
//   abn_sort_check_kernel      a lane per site: its key against its predecessor's; per workgroup the descents, the equal
//                              neighbours, the OR and the AND of the keys and the keys outside their ranges; writes the
//                              pairs with index = position
//   abn_sort_hist_kernel       a workgroup per tile: count[d * stride + tile] = the tile's pairs of digit d (integer LDS
//                              atomics: a count does not depend on arrival order)
//   abn_parse_scan_kernel      (abn_parse_kernels.hpp) a workgroup per digit: the exclusive scan of the digit's row of tile
//                              counts, the digit's total behind it
//   abn_sort_scatter_kernel    a workgroup per tile: destination = (the pairs of smaller digits: a block scan of the 256
//                              row totals) + (the digit's pairs in earlier tiles: the scanned row) + (the digit's pairs of
//                              earlier groups of the tile: LDS) + (those in front of it in its group: ballots and a
//                              popcount)
//   abn_sort_order_kernel      order[k] = the index of pair k
//   abn_sort_gather_kernel     a lane per output record: the record arrays copied from order[k], line = k
//
// Stability: within a pass the destination is strictly increasing along the input order among pairs of one digit — tile
// after tile by the scan, group after group by the prefix in LDS, lane after lane by the popcount of the lower lanes — and
// nothing in it comes from an atomic's return value.  Every output element has one writer and a plain vector store; no
// workgroup waits for another.
//
// What the choice costs: the scatter kernel keeps its 8 pairs in registers (32 VGPRs) with their digits and ranks — 76
// VGPRs in all, 6 wavefronts per SIMD, no scratch — and 17 KiB of LDS: 32 groups x 256 digits of 16-bit counts (a group
// holds at most 64, their prefix at most 2048) and 256 bases.  Nine workgroups fit the 160 KiB of a CU, more than the six
// the registers allow, so LDS never bounds occupancy.  The count table has 256 x (tiles + 1) words: 0.5 B per pair.
//
// The key layout, the digit function and the sort in its serial forms compile without a HIP header: the host library
// (host_capi.cpp) and tests/native/sites_sort_main.cpp include this file as it is.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "abn_parse.hpp"
#include "abn_sites_merge.hpp"

namespace abn {

constexpr int kSortThreads = 256;
constexpr int kSortItems = 8;
constexpr int kSortTile = kSortThreads * kSortItems;
constexpr int kSortGroups = kSortTile / 64;  // of 64 consecutive pairs: one wavefront's pairs of one item
constexpr int kSortDigitBits = 8;
constexpr int kSortDigits = 1 << kSortDigitBits;
constexpr int kSortKeyBits = 75;
constexpr int kSortPasses = (kSortKeyBits + kSortDigitBits - 1) / kSortDigitBits;  // 10
constexpr int kSortCheckBlocks = 1024;  // at most this many partial records of the check come to the host
constexpr int kSortCheckWords = 9;      // descents, equal, or[3], and[3], bad
static_assert(kSortDigits == kSortThreads, "the scatter kernel gives every digit a lane");
static_assert(32 % kSortDigitBits == 0, "no digit straddles a word of the key");

struct SortKey {
  uint32_t w[3];
};

ABN_HOST_DEVICE inline SortKey sort_key(uint32_t chromosome, uint32_t start, uint32_t end, uint32_t strand) {
  return SortKey{{strand | end << 2, end >> 30 | start << 2, start >> 30 | chromosome << 2}};
}
ABN_HOST_DEVICE inline bool sort_key_valid(int32_t chromosome, uint32_t strand) {
  return chromosome >= 0 && chromosome <= 257 && strand <= 2u;
}
ABN_HOST_DEVICE inline SortKey sort_key_of_meta(uint32_t meta, uint32_t start, uint32_t end) {
  return sort_key((uint32_t)meta_chromosome(meta), start, end, meta_strand(meta));
}
// the digit pass p sorts by: bits 8p .. 8p + 7 of the key
ABN_HOST_DEVICE inline uint32_t sort_digit(const uint32_t* w, int pass) {
  return (w[pass >> 2] >> ((pass & 3) * kSortDigitBits)) & (uint32_t)(kSortDigits - 1);
}
// -1, 0, 1: a below, equal to, above b
ABN_HOST_DEVICE inline int sort_key_compare(const uint32_t* a, const uint32_t* b) {
  for (int k = 2; k >= 0; --k)
    if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
  return 0;
}
// Pass p moves nothing when every key has the same digit there: the OR and the AND of all keys agree in its bits
ABN_HOST_DEVICE inline bool sort_pass_constant(const uint32_t* key_or, const uint32_t* key_and, int pass) {
  return sort_digit(key_or, pass) == sort_digit(key_and, pass);
}
ABN_HOST_DEVICE inline long long sort_tiles(long long n) { return (n + kSortTile - 1) / kSortTile; }

struct SortPair {  // a uint4 on the device
  uint32_t w[3];
  uint32_t index;
};

// What the check finds, added up over its workgroups' partial records
struct SortCheck {
  long long descents = 0, equal = 0, bad = 0;
  uint32_t key_or[3] = {0u, 0u, 0u}, key_and[3] = {~0u, ~0u, ~0u};
};

// ---- serial forms
// the pairs of n keys in input order, and what the check kernel reports of them
inline SortCheck sort_check_serial(long long n, const int32_t* chromosome, const uint32_t* start, const uint32_t* end,
                                   const uint8_t* strand, SortPair* pair) {
  SortCheck c;
  for (long long i = 0; i < n; ++i) {
    if (!sort_key_valid(chromosome[i], strand[i])) ++c.bad;
    const SortKey k = sort_key((uint32_t)chromosome[i], start[i], end[i], strand[i]);
    pair[i] = SortPair{{k.w[0], k.w[1], k.w[2]}, (uint32_t)i};
    for (int j = 0; j < 3; ++j) c.key_or[j] |= k.w[j], c.key_and[j] &= k.w[j];
    if (i > 0) {
      const int cmp = sort_key_compare(pair[i].w, pair[i - 1].w);
      c.descents += cmp < 0, c.equal += cmp == 0;
    }
  }
  return c;
}

// the reference form: a stable comparison sort
inline void sort_pairs_serial(SortPair* pair, long long n) {
  std::stable_sort(pair, pair + n, [](const SortPair& a, const SortPair& b) { return sort_key_compare(a.w, b.w) < 0; });
}

// One pass, workgroup by workgroup as the kernels walk it: the tile histograms, the scan of every digit's row, and the
// scatter with the rank inside the tile built from the per-group (per-wavefront) counts.  count: kSortDigits * stride
// words, stride = tiles + 1
inline void sort_pass_walk(const SortPair* in, SortPair* out, long long n, int pass, uint32_t* count, long long stride) {
  const long long tiles = sort_tiles(n);
  for (long long t = 0; t < tiles; ++t) {  // abn_sort_hist_kernel
    for (int d = 0; d < kSortDigits; ++d) count[d * stride + t] = 0u;
    for (long long i = t * kSortTile; i < n && i < (t + 1) * kSortTile; ++i) ++count[sort_digit(in[i].w, pass) * stride + t];
  }
  for (int d = 0; d < kSortDigits; ++d) {  // abn_parse_scan_kernel, a workgroup per digit
    uint32_t run = 0;
    for (long long t = 0; t <= tiles; ++t) {
      const uint32_t v = t < tiles ? count[d * stride + t] : 0u;
      count[d * stride + t] = run;
      run += v;
    }
  }
  for (long long t = 0; t < tiles; ++t) {  // abn_sort_scatter_kernel
    uint32_t base[kSortDigits], run = 0;
    for (int d = 0; d < kSortDigits; ++d) {  // the block scan of the row totals, then the row's entry of this tile
      base[d] = run + count[d * stride + t];
      run += count[d * stride + tiles];
    }
    uint16_t group[kSortGroups][kSortDigits] = {};
    for (int g = 0; g < kSortGroups; ++g)
      for (long long i = t * kSortTile + g * 64; i < n && i < t * kSortTile + (g + 1) * 64; ++i)
        ++group[g][sort_digit(in[i].w, pass)];
    for (int d = 0; d < kSortDigits; ++d) {  // exclusive over the groups
      uint16_t before = 0;
      for (int g = 0; g < kSortGroups; ++g) {
        const uint16_t v = group[g][d];
        group[g][d] = before;
        before = (uint16_t)(before + v);
      }
    }
    for (int g = 0; g < kSortGroups; ++g) {
      const long long lo = t * kSortTile + g * 64;
      for (long long i = lo; i < n && i < lo + 64; ++i) {
        const uint32_t d = sort_digit(in[i].w, pass);
        uint32_t in_wave = 0;  // the ballot's popcount below this lane
        for (long long j = lo; j < i; ++j) in_wave += sort_digit(in[j].w, pass) == d;
        out[base[d] + group[g][d] + in_wave] = in[i];
      }
    }
  }
}

// The sort as the device runs it: no pass for an input without a descent, else every pass whose digit is not constant
// (skip) or every pass (skip = false); a and b: n pairs each, a holds the input.  Returns the buffer that holds the result;
// *passes = the passes run
inline SortPair* sort_walk_serial(SortPair* a, SortPair* b, long long n, const SortCheck& check, bool skip, int* passes) {
  *passes = 0;
  if (check.descents == 0) return a;
  const long long stride = sort_tiles(n) + 1;
  std::vector<uint32_t> count((size_t)kSortDigits * (size_t)stride);
  for (int p = 0; p < kSortPasses; ++p) {
    if (skip && sort_pass_constant(check.key_or, check.key_and, p)) continue;
    sort_pass_walk(a, b, n, p, count.data(), stride);
    std::swap(a, b);
    ++*passes;
  }
  return a;
}

// the passes a sort of keys with this check runs
inline int sort_passes_needed(const SortCheck& check) {
  if (check.descents == 0) return 0;
  int passes = 0;
  for (int p = 0; p < kSortPasses; ++p) passes += sort_pass_constant(check.key_or, check.key_and, p) ? 0 : 1;
  return passes;
}

// ---- the flatten: the sample's sites in file order with their whole record
struct SortFlat {
  uint32_t* meta;
  uint32_t* start;
  uint32_t* end;
  double* posteriormax;
  double* meth_lvl;
};

// an inserted record's meta word (it has no status_flag: the host's parser printed its warning)
ABN_HOST_DEVICE inline uint32_t sort_inserted_meta(int32_t chromosome, uint32_t strand, uint32_t status, uint32_t context) {
  return (uint32_t)chromosome | strand << 16 | status << 20 | context << kMetaContextShift;
}

// one device record to its place: what a lane of abn_sort_flatten_records_kernel does
ABN_HOST_DEVICE inline long long sort_flatten_record(const MergeChunk& c, long long i, const long long* inserted_line,
                                                     long long n_inserted, const SortFlat& out) {
  const long long d = merge_dest_record(c, i, inserted_line, n_inserted);
  out.meta[d] = c.meta[i];
  out.start[d] = c.start[i];
  out.end[d] = c.end[i];
  out.posteriormax[d] = c.posteriormax[i];
  out.meth_lvl[d] = c.meth_lvl[i];
  return d;
}

// one inserted record to its place (context: every inserted record's code): a lane of abn_sort_flatten_inserted_kernel
ABN_HOST_DEVICE inline long long sort_flatten_inserted(const MergeChunk* chunks, const MergeInserted& ins,
                                                       const uint8_t* context, long long j, const SortFlat& out) {
  const long long d = merge_dest_inserted(chunks[ins.chunk[j]], j, ins.line[j]);
  out.meta[d] = sort_inserted_meta(ins.chromosome[j], ins.strand[j], ins.status[j], context[j]);
  out.start[d] = ins.start[j];
  out.end[d] = ins.end[j];
  out.posteriormax[d] = ins.posteriormax[j];
  out.meth_lvl[d] = ins.meth_lvl[j];
  return d;
}

inline void sort_flatten_serial(const MergeChunk* chunks, int n_chunks, const MergeInserted& ins, const uint8_t* context,
                                const SortFlat& out) {
  for (int c = 0; c < n_chunks; ++c)
    for (long long i = 0; i < chunks[c].n; ++i) sort_flatten_record(chunks[c], i, ins.line, ins.n, out);
  for (long long j = 0; j < ins.n; ++j) sort_flatten_inserted(chunks, ins, context, j, out);
}

// one output record from its source: what a lane of abn_sort_gather_kernel does
// (n: the records; an index outside them, which no sort of these kernels gives, copies nothing)
ABN_HOST_DEVICE inline void sort_gather_record(const SortFlat& in, const uint32_t* order, long long k, long long n,
                                               const ParseRecords& out) {
  const uint32_t i = order[k];
  if ((long long)i >= n) return;
  out.line[k] = (uint32_t)k;
  out.meta[k] = in.meta[i];
  out.start[k] = in.start[i];
  out.end[k] = in.end[i];
  out.posteriormax[k] = in.posteriormax[i];
  out.meth_lvl[k] = in.meth_lvl[i];
}

#if defined(__HIPCC__) && defined(ABN_SITES_SORT_KERNELS)  // (abn_sites_sort.hip defines it: hipcc also builds the host library)
// ------------------------------------------------------------------------------------------------ kernels
static_assert(sizeof(SortPair) == sizeof(uint4), "a pair is one 16-byte load");

// grid: ceil(chunk.n / kSortThreads)
__global__ void __launch_bounds__(kSortThreads)
abn_sort_flatten_records_kernel(MergeChunk chunk, const long long* __restrict__ inserted_line, long long n_inserted,
                                SortFlat out) {
  const long long i = (long long)blockIdx.x * kSortThreads + threadIdx.x;
  if (i < chunk.n) sort_flatten_record(chunk, i, inserted_line, n_inserted, out);
}

// grid: ceil(ins.n / kSortThreads); chunks: the sample's chunk table in device memory
__global__ void __launch_bounds__(kSortThreads)
abn_sort_flatten_inserted_kernel(const MergeChunk* __restrict__ chunks, MergeInserted ins,
                                 const uint8_t* __restrict__ context, SortFlat out) {
  const long long j = (long long)blockIdx.x * kSortThreads + threadIdx.x;
  if (j < ins.n) sort_flatten_inserted(chunks, ins, context, j, out);
}

// Where the check reads its keys: the four key arrays of the primitive, or a flattened sample's meta, start and end
struct SortKeysArrays {
  const int32_t* chromosome;
  const uint32_t* start;
  const uint32_t* end;
  const uint8_t* strand;
  __device__ __forceinline__ SortKey at(long long i, uint32_t& bad) const {
    const int32_t c = chromosome[i];
    const uint32_t s = strand[i];
    bad += sort_key_valid(c, s) ? 0u : 1u;
    return sort_key((uint32_t)c, start[i], end[i], s);
  }
};
struct SortKeysMeta {
  const uint32_t* meta;
  const uint32_t* start;
  const uint32_t* end;
  __device__ __forceinline__ SortKey at(long long i, uint32_t& bad) const {
    const uint32_t m = meta[i];
    bad += sort_key_valid(meta_chromosome(m), meta_strand(m)) ? 0u : 1u;
    return sort_key_of_meta(m, start[i], end[i]);
  }
};

// grid: at most kSortCheckBlocks workgroups striding over the n keys.  pair[i] = {key i, i}; partial[blockIdx.x *
// kSortCheckWords ..] = descents, equal neighbours, OR[3], AND[3], keys outside their ranges — of the keys the workgroup saw
template <class Keys>
__global__ void __launch_bounds__(kSortThreads)
abn_sort_check_kernel(Keys keys, long long n, uint4* __restrict__ pair, uint32_t* __restrict__ partial) {
  __shared__ uint32_t s_wave[kSortThreads / 64][kSortCheckWords];
  uint32_t v[kSortCheckWords] = {0u, 0u, 0u, 0u, 0u, ~0u, ~0u, ~0u, 0u};
  for (long long i = (long long)blockIdx.x * kSortThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kSortThreads) {
    uint32_t unused = 0;
    const SortKey k = keys.at(i, v[8]);
    pair[i] = make_uint4(k.w[0], k.w[1], k.w[2], (uint32_t)i);
#pragma unroll
    for (int j = 0; j < 3; ++j) v[2 + j] |= k.w[j], v[5 + j] &= k.w[j];
    if (i > 0) {
      const SortKey p = keys.at(i - 1, unused);
      const int cmp = sort_key_compare(k.w, p.w);
      v[0] += cmp < 0 ? 1u : 0u;
      v[1] += cmp == 0 ? 1u : 0u;
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    v[0] += __shfl_down(v[0], d, 64);
    v[1] += __shfl_down(v[1], d, 64);
    v[8] += __shfl_down(v[8], d, 64);
#pragma unroll
    for (int j = 0; j < 3; ++j) v[2 + j] |= __shfl_down(v[2 + j], d, 64), v[5 + j] &= __shfl_down(v[5 + j], d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < kSortCheckWords; ++j) s_wave[threadIdx.x >> 6][j] = v[j];
  }
  __syncthreads();
  if (threadIdx.x < kSortCheckWords) {
    const int j = threadIdx.x;
    uint32_t r = s_wave[0][j];
    for (int w = 1; w < kSortThreads / 64; ++w) {
      const uint32_t x = s_wave[w][j];
      r = (j >= 2 && j < 5) ? (r | x) : (j >= 5 && j < 8) ? (r & x) : r + x;
    }
    partial[(size_t)blockIdx.x * kSortCheckWords + j] = r;
  }
}

// grid: the tiles.  count[d * stride + blockIdx.x] = the tile's pairs of digit d in pass `pass`
__global__ void __launch_bounds__(kSortThreads)
abn_sort_hist_kernel(const uint4* __restrict__ pair, uint32_t n, int pass, uint32_t* __restrict__ count, uint32_t stride) {
  __shared__ uint32_t s_hist[kSortDigits];
  s_hist[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t* word = (const uint32_t*)pair + (pass >> 2);
  const int shift = (pass & 3) * kSortDigitBits;
  const unsigned long long base = (unsigned long long)blockIdx.x * kSortTile;
#pragma unroll
  for (int it = 0; it < kSortItems; ++it) {
    const unsigned long long i = base + (unsigned)(it * kSortThreads) + threadIdx.x;
    if (i < n) atomicAdd(&s_hist[(word[i * 4] >> shift) & (uint32_t)(kSortDigits - 1)], 1u);
  }
  __syncthreads();
  count[(size_t)threadIdx.x * stride + blockIdx.x] = s_hist[threadIdx.x];
}

// grid: the tiles (stride = tiles + 1).  off: the scanned counts — off[d * stride + t] = digit d's pairs in the tiles in
// front of t, off[d * stride + tiles] = all of digit d's.  out has room for the n pairs; every one of them is written once
__global__ void __launch_bounds__(kSortThreads)
abn_sort_scatter_kernel(const uint4* __restrict__ pair, uint32_t n, int pass, const uint32_t* __restrict__ off,
                        uint32_t stride, uint4* __restrict__ out) {
  __shared__ uint16_t s_group[kSortGroups][kSortDigits];
  __shared__ uint32_t s_base[kSortDigits];
  __shared__ uint32_t s_wave[kSortThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  {  // the groups' counts start at 0: a digit no lane of a group holds has no writer
    uint32_t* z = (uint32_t*)&s_group[0][0];
    for (int k = threadIdx.x; k < kSortGroups * kSortDigits / 2; k += kSortThreads) z[k] = 0u;
  }
  // the pairs of smaller digits: the exclusive scan of the 256 row totals, a lane per digit
  const uint32_t total = off[(size_t)threadIdx.x * stride + (stride - 1u)];
  uint32_t inc = total;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d, 64);
    if (lane >= d) inc += up;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();  // (also: the zeroes of s_group are in place)
  uint32_t smaller = inc - total;
  for (int w = 0; w < wave; ++w) smaller += s_wave[w];
  s_base[threadIdx.x] = smaller + off[(size_t)threadIdx.x * stride + blockIdx.x];

  const int word = pass >> 2, shift = (pass & 3) * kSortDigitBits;
  const unsigned long long base = (unsigned long long)blockIdx.x * kSortTile;
  uint4 mine[kSortItems];
  uint32_t digit[kSortItems], in_wave[kSortItems];
#pragma unroll
  for (int it = 0; it < kSortItems; ++it) {
    const unsigned long long i = base + (unsigned)(it * kSortThreads) + threadIdx.x;
    const bool valid = i < n;
    mine[it] = valid ? pair[i] : make_uint4(0u, 0u, 0u, 0u);
    const uint32_t w = word == 0 ? mine[it].x : (word == 1 ? mine[it].y : mine[it].z);
    const uint32_t d = (w >> shift) & (uint32_t)(kSortDigits - 1);
    unsigned long long same = __ballot(valid);  // the lanes of this wavefront that hold the same digit
#pragma unroll
    for (int b = 0; b < kSortDigitBits; ++b) {
      const unsigned long long votes = __ballot((d >> b) & 1u);
      same &= ((d >> b) & 1u) ? votes : ~votes;
    }
    digit[it] = d;
    in_wave[it] = (uint32_t)__popcll(same & below);
    if (valid && in_wave[it] == 0u) s_group[it * (kSortThreads / 64) + wave][d] = (uint16_t)__popcll(same);
  }
  __syncthreads();
  {  // a lane per digit: the groups' counts to their exclusive prefix
    uint32_t before = 0;
    for (int g = 0; g < kSortGroups; ++g) {
      const uint32_t v = s_group[g][threadIdx.x];
      s_group[g][threadIdx.x] = (uint16_t)before;
      before += v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < kSortItems; ++it) {
    const unsigned long long i = base + (unsigned)(it * kSortThreads) + threadIdx.x;
    if (i >= n) continue;
    const uint32_t d = digit[it];
    const uint32_t dst = s_base[d] + s_group[it * (kSortThreads / 64) + wave][d] + in_wave[it];
    if (dst < n) out[dst] = mine[it];  // (always, for counts that are this buffer's)
  }
}

// grid: ceil(n / kSortThreads).  order[k] = the index of pair k
__global__ void __launch_bounds__(kSortThreads)
abn_sort_order_kernel(const uint4* __restrict__ pair, long long n, uint32_t* __restrict__ order) {
  const long long k = (long long)blockIdx.x * kSortThreads + threadIdx.x;
  if (k < n) order[k] = pair[k].w;
}

// grid: ceil(n / kSortThreads)
__global__ void __launch_bounds__(kSortThreads)
abn_sort_gather_kernel(SortFlat in, const uint32_t* __restrict__ order, long long n, ParseRecords out) {
  const long long k = (long long)blockIdx.x * kSortThreads + threadIdx.x;
  if (k < n) sort_gather_record(in, order, k, n, out);
}
#endif  // kernels

}  // namespace abn
