// One resident methylome parsed under a context mask, partitioned into one resident methylome per context, on the device
// (abn_sites_split): the records of every chunk of the parent go, in file order, into the chunk of the same slab of every
// child they belong to.  A record's MEMBERSHIP is 1 << its context code (abn_parse.hpp: CG 0, CHG 1, CHH 2), or 7 for a
// row without a context (code 3: the chromatin-state / bigwig rows, which every single-context parse accepts too), both
// within the parent's mask: a context the parent was not parsed under has no child.
//
// The parent's chunks are one list of WORKGROUPS: chunk c owns the split_blocks(n_c) workgroups from block0_c on, a lane
// per record.  With count[k][b] = the records of workgroup b that belong to child k and off[k] its exclusive scan over
// all workgroups of the parent,
//
//   record i of chunk c, in workgroup b, member of child k
//     ->  slot off[k][b] - off[k][block0_c] + #{members of k in workgroup b in front of i}   of child k's chunk c
//
// which fills child k's chunk c densely and in file order; that chunk holds off[k][block0_{c+1}] - off[k][block0_c]
// records.  Every output element has one writer, found by a scan; there are no atomics and every store is a plain vector
// store.
//
//   abn_split_count_kernel    a lane per record: ballot + popcount per wavefront and child, LDS holds the wave totals only;
//                             three counts per workgroup
//   abn_parse_scan_kernel     (abn_parse_kernels.hpp) scans the three count arrays
//   abn_split_sizes_kernel    a lane per (chunk, child): the chunk's records of that child — all that comes to the host
//   abn_split_scatter_kernel  the same mapping, the ranks recomputed: the six record arrays copied to every child the record
//                             belongs to (32 B read, up to 32 B written per record and child)
//   abn_split_flagged_kernel  a lane per flagged line of the parent (rare): a lower bound in its chunk finds the record, and
//                             so the children that inherit the line
//
// The index arithmetic and the partition in its serial form compile without a HIP header: the host library
// (host_capi.cpp) and tests/native/sites_split_main.cpp include this file as it is.
#pragma once
#include <stdint.h>

#include "abn_parse.hpp"
#include "abn_sites_merge.hpp"

namespace abn {

constexpr int kSplitThreads = 256;
constexpr int kSplitChildren = 3;

using SplitOut = ParseRecords;  // one child's chunk

struct SplitChunk {
  MergeChunk src;      // the parent's chunk
  long long block0;    // its first workgroup
  SplitOut out[kSplitChildren];  // the children's chunks of the same slab (unread by the count)
};

// the children a record belongs to, as a mask; contexts: the parent's mask — only its contexts have a child
ABN_HOST_DEVICE inline uint32_t split_membership(uint32_t meta, uint32_t contexts) {
  const uint32_t code = meta_context(meta);
  return (code == kCtxNone ? kContextsAll : 1u << code) & contexts;
}

ABN_HOST_DEVICE inline long long split_blocks(long long n) { return (n + kSplitThreads - 1) / kSplitThreads; }

// the chunk that owns workgroup b: the last one whose block0 is at most b and that has a workgroup at all
ABN_HOST_DEVICE inline int split_chunk_of_block(const SplitChunk* chunks, int n_chunks, long long b) {
  int lo = 0, hi = n_chunks;  // the first chunk with block0 > b
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (chunks[mid].block0 <= b) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;  // chunks without a record share their block0 with the next one: they sort in front of it
}

// one record to slot k of one child's chunk
ABN_HOST_DEVICE inline void split_copy_record(const MergeChunk& c, long long i, const SplitOut& o, long long k) {
  o.line[k] = c.line[i];
  o.meta[k] = c.meta[i];
  o.start[k] = c.start[i];
  o.end[k] = c.end[i];
  o.posteriormax[k] = c.posteriormax[i];
  o.meth_lvl[k] = c.meth_lvl[i];
}

// the children that inherit the parent's flagged file line `line`, a line of chunk c's slab; 0: no record has that line
ABN_HOST_DEVICE inline uint32_t split_flagged_membership(const MergeChunk& c, long long line, uint32_t contexts) {
  const uint32_t rel = (uint32_t)(line - c.line0);
  const long long i = merge_lower_bound(c.line, c.n, rel);
  return (i < c.n && c.line[i] == rel) ? split_membership(c.meta[i], contexts) : 0u;
}

// ---- the partition, serially, workgroup by workgroup as the kernels walk it
// count [kSplitChildren * stride], stride > the parent's workgroups: count[k * stride + b]
inline void split_count_serial(const SplitChunk* chunks, int n_chunks, uint32_t contexts, uint32_t* count,
                               long long stride) {
  for (int c = 0; c < n_chunks; ++c)
    for (long long b = 0; b < split_blocks(chunks[c].src.n); ++b) {
      uint32_t n[kSplitChildren] = {0, 0, 0};
      for (long long i = b * kSplitThreads; i < chunks[c].src.n && i < (b + 1) * kSplitThreads; ++i) {
        const uint32_t m = split_membership(chunks[c].src.meta[i], contexts);
        for (int k = 0; k < kSplitChildren; ++k) n[k] += (m >> k) & 1u;
      }
      for (int k = 0; k < kSplitChildren; ++k) count[k * stride + chunks[c].block0 + b] = n[k];
    }
}

// abn_parse_scan_kernel for the three arrays: exclusive, the total behind the n_blocks counts
inline void split_scan_serial(uint32_t* count, long long n_blocks, long long stride) {
  for (int k = 0; k < kSplitChildren; ++k) {
    uint32_t run = 0;
    for (long long b = 0; b <= n_blocks; ++b) {
      const uint32_t v = b < n_blocks ? count[k * stride + b] : 0u;
      count[k * stride + b] = run;
      run += v;
    }
  }
}

// the records of chunk c that belong to child k, from the scanned counts (n_blocks: the parent's workgroups)
ABN_HOST_DEVICE inline uint32_t split_chunk_size(const SplitChunk* chunks, int n_chunks, int c, int k, const uint32_t* off,
                                                 long long stride, long long n_blocks) {
  const long long next = c + 1 < n_chunks ? chunks[c + 1].block0 : n_blocks;
  return off[k * stride + next] - off[k * stride + chunks[c].block0];
}

inline void split_scatter_serial(const SplitChunk* chunks, int n_chunks, uint32_t contexts, const uint32_t* off,
                                 long long stride, long long n_blocks) {
  for (long long b = 0; b < n_blocks; ++b) {
    const int c = split_chunk_of_block(chunks, n_chunks, b);
    const SplitChunk& ch = chunks[c];
    uint32_t rank[kSplitChildren];
    for (int k = 0; k < kSplitChildren; ++k) rank[k] = off[k * stride + b] - off[k * stride + ch.block0];
    for (long long i = (b - ch.block0) * kSplitThreads; i < ch.src.n && i < (b - ch.block0 + 1) * kSplitThreads; ++i) {
      const uint32_t m = split_membership(ch.src.meta[i], contexts);
      for (int k = 0; k < kSplitChildren; ++k)
        if ((m >> k) & 1u) split_copy_record(ch.src, i, ch.out[k], rank[k]++);
    }
  }
}

#if defined(__HIPCC__) && defined(ABN_SITES_SPLIT_KERNELS)  // (abn_sites.hip defines it: hipcc also builds the host library)
// ------------------------------------------------------------------------------------------------ kernels
// The record of this lane and its membership (0 behind the chunk's end); c = the workgroup's chunk
__device__ __forceinline__ uint32_t split_lane_membership(const SplitChunk* __restrict__ chunks, int n_chunks,
                                                          uint32_t contexts, int& c, long long& i) {
  c = split_chunk_of_block(chunks, n_chunks, (long long)blockIdx.x);
  i = ((long long)blockIdx.x - chunks[c].block0) * kSplitThreads + threadIdx.x;
  return i < chunks[c].src.n ? split_membership(chunks[c].src.meta[i], contexts) : 0u;
}

// grid: the parent's workgroups.  count[k * stride + blockIdx.x] = the workgroup's members of child k
__global__ void __launch_bounds__(kSplitThreads)
abn_split_count_kernel(const SplitChunk* __restrict__ chunks, int n_chunks, uint32_t contexts, uint32_t* __restrict__ count,
                       uint32_t stride) {
  __shared__ uint32_t s_wave[kSplitChildren][kSplitThreads / 64];
  int c;
  long long i;
  const uint32_t m = split_lane_membership(chunks, n_chunks, contexts, c, i);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kSplitChildren; ++k) {
    const unsigned long long votes = __ballot((m >> k) & 1u);
    if (lane == 0) s_wave[k][wave] = (uint32_t)__popcll(votes);
  }
  __syncthreads();
  if (threadIdx.x < kSplitChildren) {
    uint32_t sum = 0;
    for (int w = 0; w < kSplitThreads / 64; ++w) sum += s_wave[threadIdx.x][w];
    count[(size_t)threadIdx.x * stride + blockIdx.x] = sum;
  }
}

// grid: ceil(n_chunks * kSplitChildren / kSplitThreads).  size[c * kSplitChildren + k]; off: the scanned counts
__global__ void __launch_bounds__(kSplitThreads)
abn_split_sizes_kernel(const SplitChunk* __restrict__ chunks, int n_chunks, const uint32_t* __restrict__ off, uint32_t stride,
                       uint32_t n_blocks, uint32_t* __restrict__ size) {
  const long long t = (long long)blockIdx.x * kSplitThreads + threadIdx.x;
  if (t < (long long)n_chunks * kSplitChildren)
    size[t] = split_chunk_size(chunks, n_chunks, (int)(t / kSplitChildren), (int)(t % kSplitChildren), off, stride, n_blocks);
}

// grid: the parent's workgroups; off: the scanned counts.  chunks[c].out[k] has room for split_chunk_size(c, k) records
__global__ void __launch_bounds__(kSplitThreads)
abn_split_scatter_kernel(const SplitChunk* __restrict__ chunks, int n_chunks, uint32_t contexts,
                         const uint32_t* __restrict__ off, uint32_t stride) {
  __shared__ uint32_t s_wave[kSplitChildren][kSplitThreads / 64];
  int c;
  long long i;
  const uint32_t m = split_lane_membership(chunks, n_chunks, contexts, c, i);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t in_wave[kSplitChildren];
#pragma unroll
  for (int k = 0; k < kSplitChildren; ++k) {
    const unsigned long long votes = __ballot((m >> k) & 1u);
    in_wave[k] = (uint32_t)__popcll(votes & below);
    if (lane == 0) s_wave[k][wave] = (uint32_t)__popcll(votes);
  }
  __syncthreads();
  if (m == 0u) return;
  const SplitChunk& ch = chunks[c];
#pragma unroll
  for (int k = 0; k < kSplitChildren; ++k) {
    if (!((m >> k) & 1u)) continue;
    uint32_t rank = off[(size_t)k * stride + blockIdx.x] - off[(size_t)k * stride + ch.block0] + in_wave[k];
    for (int w = 0; w < wave; ++w) rank += s_wave[k][w];
    split_copy_record(ch.src, i, ch.out[k], (long long)rank);
  }
}

// grid: ceil(n / kSplitThreads).  line [n]: the parent's flagged file lines, chunk [n]: the chunk whose slab holds each;
// member[j] = the children that inherit line j
__global__ void __launch_bounds__(kSplitThreads)
abn_split_flagged_kernel(const SplitChunk* __restrict__ chunks, const long long* __restrict__ line,
                         const int32_t* __restrict__ chunk, long long n, uint32_t contexts,
                         uint8_t* __restrict__ member) {
  const long long j = (long long)blockIdx.x * kSplitThreads + threadIdx.x;
  if (j < n) member[j] = (uint8_t)split_flagged_membership(chunks[chunk[j]].src, line[j], contexts);
}
#endif  // kernels

}  // namespace abn
