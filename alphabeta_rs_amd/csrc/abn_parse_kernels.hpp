// Methylome text -> site records on the device (abn_sites_parse): MethylationSite::from_methylome_file_line
// (src/methylation_site.rs:146-362) for every line of a slab of text, with the line parser of abn_parse.hpp.
//
//   K1 abn_parse_count_kernel    a lane per 16-byte piece (one dwordx4 load): the '\n' bytes of the piece, summed per
//                                workgroup (4 KiB of text)
//      abn_parse_scan_kernel     one workgroup per array: exclusive scan of n counts in place, the total behind them
//   K2 abn_parse_index_kernel    the same load again; a block scan gives every '\n' its rank, and the line behind it its
//                                begin offset: line_begin[rank + 1] = position + 1
//   K3 abn_parse_lines_kernel    a workgroup per run of kParseRun consecutive lines: their contiguous bytes staged into
//                                LDS with dwordx4 loads, a lane per line parsing from LDS; a block scan over "site" and
//                                "deferred" stores both kinds densely per run, the run's counts beside them
//   K4 abn_parse_compact_kernel  after the scan of the runs' counts: every run's records to their final slots
// Order is file order by construction: every output element has one writer, found by a scan; there are no atomics, and
// every store is a plain vector store.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "abn_parse.hpp"

namespace abn {

constexpr int kParseThreads = 256;
constexpr int kParsePieceBytes = 16;
constexpr int kParseBlockBytes = kParseThreads * kParsePieceBytes;  // text per workgroup of K1 / K2
constexpr int kParseRun = 256;                                      // lines per workgroup of K3, one per lane
// The stage: 64 bytes per line of a run — all-context methylome lines have 35 to 50.  With the run's 257 begin offsets
// and the scan's wave totals a workgroup holds 17.3 KiB of LDS: nine workgroups (36 wavefronts) fit the 160 KiB of a CU,
// more than the 32 wavefronts its SIMDs hold, so the stage never bounds occupancy.
constexpr int kParseStageBytes = 16384;
constexpr int kParseScanThreads = 1024;
static_assert(kParseStageBytes % kParsePieceBytes == 0 && kParseRun == kParseThreads, "whole pieces; a lane per line");

// the number of bytes of x that are '\n' (exact: no carry crosses a byte)
__device__ __forceinline__ uint32_t parse_newlines(uint32_t x) {
  const uint32_t y = x ^ 0x0a0a0a0au;
  const uint32_t t = ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu);  // 0x80 in every byte of y that is 0
  return (uint32_t)__popc(t);
}

// exclusive scan of v over the workgroup's kParseThreads lanes; total = the sum.  s_wave: one word per wavefront
__device__ __forceinline__ uint32_t parse_block_scan(uint32_t v, uint32_t* s_wave, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(inc, d, 64);
    if (lane >= d) inc += up;
  }
  __syncthreads();  // s_wave may still be read from the previous scan
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int w = 0; w < kParseThreads / 64; ++w) {
    const uint32_t t = s_wave[w];
    before += w < wave ? t : 0u;
    all += t;
  }
  total = all;
  return before + inc - v;
}

// K1.  text: n_pieces pieces, the bytes behind the text's end zero
__global__ void __launch_bounds__(kParseThreads)
abn_parse_count_kernel(const uint4* __restrict__ text, uint32_t n_pieces, uint32_t* __restrict__ block_count) {
  __shared__ uint32_t s_wave[kParseThreads / 64];
  const uint32_t piece = blockIdx.x * kParseThreads + threadIdx.x;
  uint32_t n = 0;
  if (piece < n_pieces) {
    const uint4 v = text[piece];
    n = parse_newlines(v.x) + parse_newlines(v.y) + parse_newlines(v.z) + parse_newlines(v.w);
  }
  uint32_t total;
  (void)parse_block_scan(n, s_wave, total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// Workgroup a scans the n counts at data + a * stride in place (exclusive) and writes their sum to entry n.
__global__ void __launch_bounds__(kParseScanThreads)
abn_parse_scan_kernel(uint32_t* __restrict__ data, uint32_t n, uint32_t stride) {
  __shared__ uint32_t s_part[kParseScanThreads];
  uint32_t* a = data + (size_t)blockIdx.x * stride;
  const uint32_t per = (n + kParseScanThreads - 1) / kParseScanThreads;
  const uint32_t lo = min(threadIdx.x * per, n), hi = min(lo + per, n);
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += a[i];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < kParseScanThreads; d <<= 1) {  // Hillis-Steele, inclusive
    const uint32_t up = threadIdx.x >= (unsigned)d ? s_part[threadIdx.x - d] : 0u;
    __syncthreads();
    s_part[threadIdx.x] += up;
    __syncthreads();
  }
  uint32_t run = s_part[threadIdx.x] - sum;
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t c = a[i];
    a[i] = run;
    run += c;
  }
  if (threadIdx.x == kParseScanThreads - 1) a[n] = s_part[threadIdx.x];
}

// K2.  block_off: K1's counts after the scan.  line_begin has (number of '\n') + 1 entries: line 0 begins at 0, the line
// behind the '\n' of rank r at that byte's position + 1 (for a text that ends in '\n' the last entry is the text's
// length: the end of the last line, not the begin of another).
__global__ void __launch_bounds__(kParseThreads)
abn_parse_index_kernel(const uint4* __restrict__ text, uint32_t n_pieces, const uint32_t* __restrict__ block_off,
                       uint32_t* __restrict__ line_begin) {
  __shared__ uint32_t s_wave[kParseThreads / 64];
  const uint32_t piece = blockIdx.x * kParseThreads + threadIdx.x;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (piece < n_pieces) v = text[piece];
  const uint32_t n = parse_newlines(v.x) + parse_newlines(v.y) + parse_newlines(v.z) + parse_newlines(v.w);
  uint32_t total;
  uint32_t rank = block_off[blockIdx.x] + parse_block_scan(n, s_wave, total);
  if (blockIdx.x == 0 && threadIdx.x == 0) line_begin[0] = 0;
  if (n == 0) return;
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (((w[d] >> (8 * k)) & 0xffu) == 0x0au) line_begin[++rank] = piece * kParsePieceBytes + 4 * d + k + 1;
}

// K3.  (ParseRecords, ParseDeferred and the meta word: abn_parse.hpp.)  The slab has n_lines lines, n_newlines of them ended by '\n' (line_begin has n_newlines + 1 entries); the lines
// from first_line on are parsed, kParseRun per workgroup.  Line l is [begin(l), begin(l + 1) - 1), where begin(l) for
// l > n_newlines is n_bytes + 1 (the last line has no '\n').  A run whose bytes exceed the stage is staged in several
// cuts of whole lines; a line that alone exceeds it is deferred unread.  The run's records go to rec / def at
// run * kParseRun + (rank in the run), its counts to run_count[run] and run_count[count_stride + run].
__global__ void __launch_bounds__(kParseThreads)
abn_parse_lines_kernel(const uint4* __restrict__ text, uint32_t n_bytes, const uint32_t* __restrict__ line_begin,
                       uint32_t n_newlines, uint32_t n_lines, uint32_t first_line, uint32_t contexts, ParseRecords rec,
                       ParseDeferred def, uint32_t* __restrict__ run_count, uint32_t count_stride) {
  __shared__ uint4 s_stage[kParseStageBytes / kParsePieceBytes];
  __shared__ uint32_t s_begin[kParseRun + 1];
  __shared__ uint32_t s_wave[kParseThreads / 64];
  const uint32_t line0 = first_line + blockIdx.x * kParseRun;
  for (uint32_t t = threadIdx.x; t <= kParseRun; t += kParseThreads) {
    const uint32_t l = min(line0 + t, n_lines);
    s_begin[t] = l <= n_newlines ? line_begin[l] : n_bytes + 1u;
  }
  __syncthreads();
  const uint32_t in_run = min((uint32_t)kParseRun, n_lines - line0);
  const uint32_t b = s_begin[threadIdx.x], e = s_begin[threadIdx.x + 1] - 1u;  // (unused beyond in_run)
  int cls = kLineNone;
  ParsedSite site{};
  uint32_t def_len = 0;
  uint32_t s = 0;  // the first line of the run not yet decided; uniform over the workgroup
  while (s < in_run) {
    const uint32_t base = s_begin[s] & ~(uint32_t)(kParsePieceBytes - 1);
    const bool fits = threadIdx.x >= s && threadIdx.x < in_run && e - base <= (uint32_t)kParseStageBytes;
    const uint32_t cnt = (uint32_t)__syncthreads_count(fits ? 1 : 0);  // line ends ascend: the lines that fit are a prefix
    if (cnt == 0) {  // line s alone is longer than the stage
      if (threadIdx.x == s) {
        cls = kLineDeferred;
        const unsigned char* g = (const unsigned char*)text;
        def_len = (e > b && g[e - 1] == '\r') ? e - b - 1u : e - b;
      }
      ++s;
      continue;
    }
    const uint32_t pieces = (s_begin[s + cnt] - 1u - base + kParsePieceBytes - 1) / kParsePieceBytes;
    for (uint32_t t = threadIdx.x; t < pieces; t += kParseThreads) s_stage[t] = text[base / kParsePieceBytes + t];
    __syncthreads();
    if (fits) {
      const unsigned char* lb = (const unsigned char*)s_stage + (b - base);
      const unsigned char* le = abn_line_trim(lb, lb + (e - b));
      cls = abn_parse_line(lb, le, site, contexts);
      def_len = (uint32_t)(le - lb);
    }
    s += cnt;
    __syncthreads();  // the stage is overwritten by the next cut
  }
  // both kinds ranked by one scan: sites in the low half-word, deferred lines in the high one (at most kParseRun each)
  uint32_t total;
  const uint32_t ranks = parse_block_scan((cls == kLineSite ? 1u : 0u) | (cls == kLineDeferred ? 0x10000u : 0u), s_wave, total);
  const size_t slot0 = (size_t)blockIdx.x * kParseRun;
  if (cls == kLineSite) {
    const size_t k = slot0 + (ranks & 0xffffu);
    rec.line[k] = line0 + threadIdx.x;
    rec.meta[k] = meta_pack(site);
    rec.start[k] = site.start;
    rec.end[k] = site.end;
    rec.posteriormax[k] = site.posteriormax;
    rec.meth_lvl[k] = site.meth_lvl;
  } else if (cls == kLineDeferred) {
    const size_t k = slot0 + (ranks >> 16);
    def.line[k] = line0 + threadIdx.x;
    def.offset[k] = b;
    def.length[k] = def_len;
  }
  if (threadIdx.x == 0) {
    run_count[blockIdx.x] = total & 0xffffu;
    run_count[count_stride + blockIdx.x] = total >> 16;
  }
}

// K4.  run_off: K3's counts after the scan (count_stride apart, each with its total behind the last run)
__global__ void __launch_bounds__(kParseThreads)
abn_parse_compact_kernel(ParseRecords from, ParseDeferred dfrom, const uint32_t* __restrict__ run_off,
                         uint32_t count_stride, ParseRecords to, ParseDeferred dto) {
  const size_t slot = (size_t)blockIdx.x * kParseRun + threadIdx.x;
  const uint32_t o = run_off[blockIdx.x], n = run_off[blockIdx.x + 1] - o;
  if (threadIdx.x < n) {
    const size_t k = (size_t)o + threadIdx.x;
    to.line[k] = from.line[slot];
    to.meta[k] = from.meta[slot];
    to.start[k] = from.start[slot];
    to.end[k] = from.end[slot];
    to.posteriormax[k] = from.posteriormax[slot];
    to.meth_lvl[k] = from.meth_lvl[slot];
  }
  const uint32_t d = run_off[count_stride + blockIdx.x], nd = run_off[count_stride + blockIdx.x + 1] - d;
  if (threadIdx.x < nd) {
    const size_t k = (size_t)d + threadIdx.x;
    dto.line[k] = dfrom.line[slot];
    dto.offset[k] = dfrom.offset[slot];
    dto.length[k] = dfrom.length[slot];
  }
}

}  // namespace abn
