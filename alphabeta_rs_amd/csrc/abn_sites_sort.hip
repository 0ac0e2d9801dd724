// abn_sites_sort_keys*: the stable radix sort of one sample's keys by (chromosome, start, end, strand) on the device, and
// what abn_sites_sort (abn_sites.hip) launches around it — the flatten of a resident handle into flat record arrays and
// the gather of the sorted records.  Kernels, key layout and the serial forms: abn_sites_sort.hpp; the row scan is
// abn_parse_scan_kernel, launched by abn_sites.hip (sites_scan_rows).
#define ABN_SITES_SORT_KERNELS
#include "abn_host.hpp"

using namespace abn;

namespace {

unsigned sort_grid(long long n) { return (unsigned)((n + kSortThreads - 1) / kSortThreads); }

// The check and the passes over n keys read through `keys`; dorder [n] receives the permutation.  info4 = {n, descents,
// equal neighbours, passes run}; ms2 = the HIP-event ms of the check and of the passes (with the order's copy-out).  A key
// outside its ranges, which the check kernel counts, is refused before any pass.  Returns after completion.
template <class Keys>
int sort_run(abn_ctx* c, long long n, const Keys& keys, uint32_t* dorder, int64_t* info4, double* ms2) {
  info4[0] = n, info4[1] = info4[2] = info4[3] = 0;
  ms2[0] = ms2[1] = 0.0;
  if (n == 0) return ABN_OK;
  const long long tiles = sort_tiles(n);
  const uint32_t stride = (uint32_t)tiles + 1u;
  const unsigned check_blocks = std::min<unsigned>(kSortCheckBlocks, sort_grid(n));
  DevBuf<uint4> a, b;
  DevBuf<uint32_t> dpartial, dcount;
  Events<4> ev;  // around the check; around the passes (the host reads the check and allocates in between)
  HIPCHK(c, a.alloc((size_t)n));
  HIPCHK(c, dpartial.alloc((size_t)check_blocks * kSortCheckWords));
  if (int rc = ev.create(c)) return rc;
  if (int rc = ev.record(c, 0)) return rc;
  hipLaunchKernelGGL(abn_sort_check_kernel<Keys>, dim3(check_blocks), dim3(kSortThreads), 0, c->stream, keys, n, a.p,
                     dpartial.p);
  HIPCHK(c, hipGetLastError());
  if (int rc = ev.record(c, 1)) return rc;
  std::vector<uint32_t> partial((size_t)check_blocks * kSortCheckWords);
  if (int rc = to_host(c, partial.data(), dpartial)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  SortCheck check;
  for (unsigned g = 0; g < check_blocks; ++g) {
    const uint32_t* p = &partial[(size_t)g * kSortCheckWords];
    check.descents += p[0], check.equal += p[1], check.bad += p[8];
    for (int j = 0; j < 3; ++j) check.key_or[j] |= p[2 + j], check.key_and[j] &= p[5 + j];
  }
  if (check.bad) return set_err(c, ABN_ERR_INVALID_ARG, "a chromosome outside 0..257 or a strand above 2");
  info4[1] = check.descents, info4[2] = check.equal;
  uint4 *src = a.p, *dst = nullptr;
  if (check.descents > 0) {
    HIPCHK(c, b.alloc((size_t)n));
    HIPCHK(c, dcount.alloc((size_t)kSortDigits * stride));
    dst = b.p;
  }
  if (int rc = ev.record(c, 2)) return rc;
  if (check.descents > 0) {
    for (int p = 0; p < kSortPasses; ++p) {
      if (sort_pass_constant(check.key_or, check.key_and, p)) continue;
      hipLaunchKernelGGL(abn_sort_hist_kernel, dim3((unsigned)tiles), dim3(kSortThreads), 0, c->stream, (const uint4*)src,
                         (uint32_t)n, p, dcount.p, stride);
      HIPCHK(c, hipGetLastError());
      if (int rc = sites_scan_rows(c, dcount.p, kSortDigits, (uint32_t)tiles, stride)) return rc;
      hipLaunchKernelGGL(abn_sort_scatter_kernel, dim3((unsigned)tiles), dim3(kSortThreads), 0, c->stream, (const uint4*)src,
                         (uint32_t)n, p, (const uint32_t*)dcount.p, stride, dst);
      HIPCHK(c, hipGetLastError());
      std::swap(src, dst);
      ++info4[3];
    }
  }
  hipLaunchKernelGGL(abn_sort_order_kernel, dim3(sort_grid(n)), dim3(kSortThreads), 0, c->stream, (const uint4*)src, n, dorder);
  HIPCHK(c, hipGetLastError());
  if (int rc = ev.record(c, 3)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int rc = ev.elapsed_ms(c, 0, &ms2[0])) return rc;
  return ev.elapsed_ms(c, 2, &ms2[1]);
}

int sort_keys_args(abn_ctx* c, int64_t n, const void* chromosome, const void* start, const void* end, const void* strand,
                   const void* order, const void* info4) {
  if (n < 0 || !info4 || (n > 0 && (!chromosome || !start || !end || !strand || !order)))
    return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n >= (int64_t)1 << 32) return set_err(c, ABN_ERR_INVALID_ARG, "abn_sites_sort_keys: 2^32 keys or more");
  return ABN_OK;
}

}  // namespace

int abn::sort_flat_dev(abn_ctx* c, long long n, const SortFlat& flat, uint32_t* dorder, int64_t* info4, double* ms2) {
  return sort_run(c, n, SortKeysMeta{flat.meta, flat.start, flat.end}, dorder, info4, ms2);
}

int abn::sort_flatten_records_dev(abn_ctx* c, const MergeChunk& chunk, const long long* dinserted_line, long long n_inserted,
                                  const SortFlat& out) {
  if (chunk.n == 0) return ABN_OK;
  hipLaunchKernelGGL(abn_sort_flatten_records_kernel, dim3(sort_grid(chunk.n)), dim3(kSortThreads), 0, c->stream, chunk,
                     dinserted_line, n_inserted, out);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

int abn::sort_flatten_inserted_dev(abn_ctx* c, const MergeChunk* dchunks, const MergeInserted& ins, const uint8_t* dcontext,
                                   const SortFlat& out) {
  if (ins.n == 0) return ABN_OK;
  hipLaunchKernelGGL(abn_sort_flatten_inserted_kernel, dim3(sort_grid(ins.n)), dim3(kSortThreads), 0, c->stream, dchunks, ins,
                     dcontext, out);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

int abn::sort_gather_dev(abn_ctx* c, const SortFlat& in, const uint32_t* dorder, long long n, const ParseRecords& out) {
  if (n == 0) return ABN_OK;
  hipLaunchKernelGGL(abn_sort_gather_kernel, dim3(sort_grid(n)), dim3(kSortThreads), 0, c->stream, in, dorder, n, out);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

extern "C" int abn_sites_sort_keys_dev(abn_ctx* c, int64_t n, const void* dchromosome, const void* dstart, const void* dend,
                                       const void* dstrand, void* dorder, int64_t* info4, double* ms2) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = sort_keys_args(c, n, dchromosome, dstart, dend, dstrand, dorder, info4)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  double ms[2];
  try {
    if (int rc = sort_run(c, n, SortKeysArrays{(const int32_t*)dchromosome, (const uint32_t*)dstart, (const uint32_t*)dend,
                                               (const uint8_t*)dstrand},
                          (uint32_t*)dorder, info4, ms))
      return rc;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  if (ms2) ms2[0] = ms[0], ms2[1] = ms[1];
  return ABN_OK;
}

extern "C" int abn_sites_sort_keys(abn_ctx* c, int64_t n, const int32_t* chromosome, const uint32_t* start,
                                   const uint32_t* end, const uint8_t* strand, int64_t* order, int64_t* info4) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = sort_keys_args(c, n, chromosome, start, end, strand, order, info4)) return rc;
  for (int64_t i = 0; i < n; ++i)  // host-only, before any launch
    if (!sort_key_valid(chromosome[i], strand[i]))
      return set_err(c, ABN_ERR_INVALID_ARG, "a chromosome outside 0..257 or a strand above 2");
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  try {
    const size_t N = (size_t)n;
    SiteKeys key;
    DevBuf<uint32_t> dorder;
    std::vector<uint32_t> o(N);
    double ms[2];
    if (int rc = key.upload(c, N, chromosome, start, end, strand)) return rc;
    HIPCHK(c, dorder.alloc(N));
    if (int rc = sort_run(c, n, SortKeysArrays{key.chrom.p, key.start.p, key.end.p, key.strand.p}, dorder.p, info4, ms)) return rc;
    if (N > 0) {
      if (int rc = to_host(c, o.data(), dorder)) return rc;
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (size_t k = 0; k < N; ++k) order[k] = (int64_t)o[k];
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  return ABN_OK;
}
