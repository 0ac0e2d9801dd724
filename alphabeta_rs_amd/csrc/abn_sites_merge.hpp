// The parser's records merged with the host-decided lines, on the device (abn_sites_parse_dev, abn_sites_insert,
// abn_windows_create_parsed): the merge by line number of windows::parse_sites_device (the loop of src/windows.rs:303-338
// over the lines of one file) and the field copy of windows::site_arrays, without a host copy of any record.
//
// A sample (one methylome) is a list of CHUNKS, one per slab of its text, in file order.  Chunk c holds the n_c records the
// device accepted in that slab — compacted, in file order, as abn_parse_compact_kernel wrote them — with slab-relative u32
// line numbers; line0_c is the file line of the slab's first line, before_c = n_0 + .. + n_{c-1}.  The INSERTED records
// are the deferred lines the host's parser accepted, sorted by file line, each with the chunk whose slab holds its line.
// A file line is a device record, a deferred line, or no site, never two of them, so
//
//   device record i of chunk c, file line l   ->  before_c + i + #{inserted lines < l}
//   inserted record j, file line l in chunk c ->  j + before_c + #{records of chunk c with a line < l}
//
// is a permutation of 0 .. n_records + n_inserted - 1 in file order.  Both counts are lower-bound binary searches over a
// sorted array; every output element has exactly one writer, a plain vector store; there are no atomics.
//
//   abn_sites_fields_kernel   a lane per device record of one chunk
//   abn_sites_insert_kernel   a lane per inserted record of one sample
//   abn_sites_flagged_kernel  the number of records of one chunk whose status byte was none of M, I, U (status_flag), as
//                             per-workgroup partial counts the host adds up
//
// The arithmetic and the merge in its serial form compile without a HIP header: the host library (host_capi.cpp) and
// tests/native/sites_merge_main.cpp include this file as it is.
#pragma once
#include <stdint.h>

#include "abn_parse.hpp"

namespace abn {

constexpr int kMergeThreads = 256;
constexpr int kMergeFlagBlocks = 256;  // at most this many partial counts per chunk

struct MergeChunk {  // the device records of one slab (ParseRecords of abn_parse.hpp, read-only)
  const uint32_t* line;  // slab-relative, strictly ascending
  const uint32_t* meta;  // (abn_parse.hpp: meta_chromosome and the accessors beside it)
  const uint32_t* start;
  const uint32_t* end;
  const double* posteriormax;
  const double* meth_lvl;
  long long n;        // records
  long long line0;    // the file line of the slab's first line
  long long n_lines;  // lines of the slab: it holds the file lines [line0, line0 + n_lines)
  long long before;   // records of the sample's chunks in front of this one
};

struct MergeInserted {  // the host-decided records of one sample, sorted by line
  const long long* line;  // file lines
  const int32_t* chunk;   // the chunk whose slab holds the line
  const int32_t* chromosome;
  const uint32_t* start;
  const uint32_t* end;
  const uint8_t* strand;
  const uint8_t* status;
  const double* posteriormax;
  const double* meth_lvl;
  long long n;
};

struct MergeOut {  // what abn_genes_choose_dev and the window placement read, at the sample's first site
  int32_t* chromosome;
  uint32_t* start;
  uint32_t* end;
  uint8_t* strand;
  uint8_t* code;
  double* level;
};

// the byte of abn_pairwise_divergence (choose_gene, host/windows_extract.hpp): the host's `<`, so a NaN posterior is kept
ABN_HOST_DEVICE inline uint8_t merge_code(uint32_t status, double posteriormax, double filter) {
  return (uint8_t)(status | (posteriormax < filter ? 0x80u : 0u));
}

// the number of entries of the ascending a[0 .. n) below key
template <class T>
ABN_HOST_DEVICE inline long long merge_lower_bound(const T* a, long long n, T key) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// where device record i of a chunk goes among the sample's sites
ABN_HOST_DEVICE inline long long merge_dest_record(const MergeChunk& c, long long i, const long long* inserted_line,
                                                   long long n_inserted) {
  return c.before + i + merge_lower_bound(inserted_line, n_inserted, c.line0 + (long long)c.line[i]);
}

// where inserted record j, whose file line lies in chunk c's slab, goes
ABN_HOST_DEVICE inline long long merge_dest_inserted(const MergeChunk& c, long long j, long long file_line) {
  return j + c.before + merge_lower_bound(c.line, c.n, (uint32_t)(file_line - c.line0));
}

// one device record to its place: what a lane of abn_sites_fields_kernel does
ABN_HOST_DEVICE inline long long merge_write_record(const MergeChunk& c, long long i, const long long* inserted_line,
                                                    long long n_inserted, double filter, const MergeOut& out) {
  const long long d = merge_dest_record(c, i, inserted_line, n_inserted);
  const uint32_t m = c.meta[i];
  out.chromosome[d] = meta_chromosome(m);
  out.start[d] = c.start[i];
  out.end[d] = c.end[i];
  out.strand[d] = (uint8_t)meta_strand(m);
  out.code[d] = merge_code(meta_status(m), c.posteriormax[i], filter);
  out.level[d] = c.meth_lvl[i];
  return d;
}

// one inserted record to its place: what a lane of abn_sites_insert_kernel does
ABN_HOST_DEVICE inline long long merge_write_inserted(const MergeChunk* chunks, const MergeInserted& ins, long long j,
                                                      double filter, const MergeOut& out) {
  const long long d = merge_dest_inserted(chunks[ins.chunk[j]], j, ins.line[j]);
  out.chromosome[d] = ins.chromosome[j];
  out.start[d] = ins.start[j];
  out.end[d] = ins.end[j];
  out.strand[d] = ins.strand[j];
  out.code[d] = merge_code(ins.status[j], ins.posteriormax[j], filter);
  out.level[d] = ins.meth_lvl[j];
  return d;
}

// The chunk of every inserted line (ascending): the one whose slab holds it.  false: a line in no chunk's slab, or the
// lines are not strictly ascending.
inline bool merge_pick_chunks(const MergeChunk* chunks, int n_chunks, const long long* line, long long n, int32_t* chunk) {
  int c = 0;
  for (long long j = 0; j < n; ++j) {
    if (j > 0 && line[j] <= line[j - 1]) return false;
    while (c < n_chunks && line[j] >= chunks[c].line0 + chunks[c].n_lines) ++c;
    if (c == n_chunks || line[j] < chunks[c].line0) return false;
    chunk[j] = c;
  }
  return true;
}

// The whole merge of one sample, serially: every chunk's records, then the inserted records.  dest_record [records of all
// chunks] and dest_inserted [ins.n] (both nullable) receive the places.
inline void sites_merge_serial(const MergeChunk* chunks, int n_chunks, const MergeInserted& ins, double filter,
                               const MergeOut& out, long long* dest_record, long long* dest_inserted) {
  for (int c = 0; c < n_chunks; ++c)
    for (long long i = 0; i < chunks[c].n; ++i) {
      const long long d = merge_write_record(chunks[c], i, ins.line, ins.n, filter, out);
      if (dest_record) dest_record[chunks[c].before + i] = d;
    }
  for (long long j = 0; j < ins.n; ++j) {
    const long long d = merge_write_inserted(chunks, ins, j, filter, out);
    if (dest_inserted) dest_inserted[j] = d;
  }
}

#if defined(__HIPCC__) && defined(ABN_SITES_MERGE_KERNELS)  // (abn_sites.hip defines it: hipcc also builds the host library)
// ------------------------------------------------------------------------------------------------ kernels
// grid: ceil(chunk.n / kMergeThreads)
__global__ void __launch_bounds__(kMergeThreads)
abn_sites_fields_kernel(MergeChunk chunk, const long long* __restrict__ inserted_line, long long n_inserted, double filter,
                        MergeOut out) {
  const long long i = (long long)blockIdx.x * kMergeThreads + threadIdx.x;
  if (i < chunk.n) merge_write_record(chunk, i, inserted_line, n_inserted, filter, out);
}

// grid: ceil(ins.n / kMergeThreads); chunks: the sample's chunk table in device memory
__global__ void __launch_bounds__(kMergeThreads)
abn_sites_insert_kernel(const MergeChunk* __restrict__ chunks, MergeInserted ins, double filter, MergeOut out) {
  const long long j = (long long)blockIdx.x * kMergeThreads + threadIdx.x;
  if (j < ins.n) merge_write_inserted(chunks, ins, j, filter, out);
}

// grid: at most kMergeFlagBlocks workgroups striding over meta[0 .. n); partial[blockIdx.x] = the flagged records it saw
__global__ void __launch_bounds__(kMergeThreads)
abn_sites_flagged_kernel(const uint32_t* __restrict__ meta, long long n, uint32_t* __restrict__ partial) {
  __shared__ uint32_t s_wave[kMergeThreads / 64];
  uint32_t count = 0;
  for (long long i = (long long)blockIdx.x * kMergeThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kMergeThreads)
    count += meta_status_flag(meta[i]) ? 1u : 0u;
  for (int d = 32; d > 0; d >>= 1) count += __shfl_down(count, d, 64);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
    for (int w = 0; w < kMergeThreads / 64; ++w) sum += s_wave[w];
    partial[blockIdx.x] = sum;
  }
}
#endif  // kernels

}  // namespace abn
