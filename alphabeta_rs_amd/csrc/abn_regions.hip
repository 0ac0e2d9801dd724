// abn_packed_region_states*: region-level methylation states of a packed matrix, and abn_regions_*: what a tiles handle's
// region matrix reports (abn_tiles_region_states, abn_tiles.hip, makes it).  The law, the kernel and its host forms:
// abn_regions.hpp.  The long windows go through the census's launcher (abn_pairwise.hip), the scans of a region matrix
// through the packed windows scans' (abn_host.hpp).
#include "abn_host.hpp"
#define ABN_REGIONS_KERNELS
#include "abn_regions.hpp"

using namespace abn;

// The body of region_states_on_device.  win, lb, le: the plan; dwin, dsrc, dtable: the launch's device buffers.  The caller
// keeps all of them until the stream has been waited for, whichever way this returns.
static int region_states_launch(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites, int64_t row_stride_bytes,
                                const std::vector<RegionWindow>& win, const std::vector<int64_t>& lb, const std::vector<int64_t>& le,
                                const int32_t* src, int64_t n_columns, const RegionRule rule, void* dev_out, int64_t out_stride,
                                double* ms2, DevBuf<RegionWindow>& dwin, DevBuf<int32_t>& dsrc,
                                DevBuf<unsigned long long>& dtable) {
  const size_t K = lb.size();
  if (int rc = upload(c, dwin, win.data(), win.size())) return rc;
  if (src)
    if (int rc = upload(c, dsrc, src, (size_t)n_columns)) return rc;
  if (K > 0) {  // one call of the census over just the long windows (it waits)
    HIPCHK(c, dtable.alloc(K * (size_t)n_samples * 3));
    if (int rc = packed_census_windows_dev(c, dev_packed, n_samples, n_sites, row_stride_bytes, lb.data(), le.data(), (int32_t)K,
                                           dtable.p, ms2 ? &ms2[0] : nullptr))
      return rc;
  }
  EventPair ev;
  if (int rc = ev.begin(c, ms2 != nullptr)) return rc;
  const dim3 grid((unsigned)(abn_packed_row_stride(n_columns) / 64), (unsigned)n_samples);
  hipLaunchKernelGGL(abn_region_states_kernel, grid, dim3(kRegionThreads), 0, c->stream, (const uint8_t*)dev_packed,
                     (long long)row_stride_bytes, (long long)n_samples, (const int32_t*)dsrc.p, (const RegionWindow*)dwin.p,
                     (const unsigned long long*)dtable.p, (long long)n_columns, rule, (uint8_t*)dev_out, (long long)out_stride);
  HIPCHK(c, hipGetLastError());
  return ev.end(c, ms2 ? &ms2[1] : nullptr);
}

int abn::region_states_on_device(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites, int64_t row_stride_bytes,
                                 const int64_t* site_begin, const int64_t* site_end, int64_t n_windows, const int32_t* src,
                                 int64_t n_columns, int64_t lo_num, int64_t hi_num, int64_t den, int64_t min_kept,
                                 int64_t long_sites, void* dev_out, int64_t out_stride, double* ms2) {
  if (ms2) ms2[0] = ms2[1] = 0.0;
  if (n_columns == 0) return ABN_OK;
  const RegionRule rule{(uint64_t)lo_num, (uint64_t)hi_num, (uint64_t)den, (uint64_t)min_kept};
  std::vector<RegionWindow> win;
  std::vector<int64_t> lb, le;
  region_plan(site_begin, site_end, n_windows, long_sites, win, lb, le);
  DevBuf<RegionWindow> dwin;
  DevBuf<int32_t> dsrc;
  DevBuf<unsigned long long> dtable;
  const int rc = region_states_launch(c, dev_packed, n_samples, n_sites, row_stride_bytes, win, lb, le, src, n_columns, rule, dev_out,
                                      out_stride, ms2, dwin, dsrc, dtable);
  // on every way out, a refusal or a HIP error included: the host's records (win, the caller's src) and the device buffers
  // of the launch stay until the stream has read them
  const hipError_t e = hipStreamSynchronize(c->stream);
  if (rc) return rc;
  HIPCHK(c, e);
  return ABN_OK;
}

// the refusals both entries share; dev: the matrix is the device's
static int region_check(abn_ctx* c, const void* packed, bool dev, int32_t n, int64_t L, int64_t stride, const int64_t* begin,
                        const int64_t* end, int64_t T, const int32_t* src, int64_t C, int64_t lo_num, int64_t hi_num, int64_t den,
                        int64_t min_kept, int64_t long_sites, const void* out) {
  const std::string why = region_refusal(packed, n, L, stride, begin, end, T, src, C, lo_num, hi_num, den, min_kept, long_sites, out);
  if (!why.empty()) return set_err(c, ABN_ERR_INVALID_ARG, why);
  if (dev && (uintptr_t)packed % 16 != 0) return set_err(c, ABN_ERR_INVALID_ARG, "dev_packed is not 16-byte aligned");
  return ABN_OK;
}

extern "C" int abn_packed_region_states_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                            int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                                            int64_t n_windows, const int32_t* src, int64_t n_columns, int64_t lo_num,
                                            int64_t hi_num, int64_t den, int64_t min_kept, int64_t long_sites, void* dev_out,
                                            double* ms2) {
  if (!c) return ABN_ERR_INVALID_ARG;
  try {
    if (int rc = region_check(c, dev_packed, true, n_samples, n_sites, row_stride_bytes, site_begin, site_end, n_windows, src,
                              n_columns, lo_num, hi_num, den, min_kept, long_sites, dev_out))
      return rc;
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    return region_states_on_device(c, dev_packed, n_samples, n_sites, row_stride_bytes, site_begin, site_end, n_windows, src,
                                   n_columns, lo_num, hi_num, den, min_kept, region_long_sites(long_sites), dev_out,
                                   abn_packed_row_stride(n_columns), ms2);
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_packed_region_states(abn_ctx* c, const uint8_t* packed, int32_t n_samples, int64_t n_sites,
                                        int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                                        int64_t n_windows, const int32_t* src, int64_t n_columns, int64_t lo_num, int64_t hi_num,
                                        int64_t den, int64_t min_kept, int64_t long_sites, uint8_t* out_packed) {
  if (!c) return ABN_ERR_INVALID_ARG;
  try {
    if (int rc = region_check(c, packed, false, n_samples, n_sites, row_stride_bytes, site_begin, site_end, n_windows, src,
                              n_columns, lo_num, hi_num, den, min_kept, long_sites, out_packed))
      return rc;
    if (n_columns == 0) return ABN_OK;
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    const size_t bytes = (size_t)n_samples * (size_t)row_stride_bytes;
    const int64_t out_stride = abn_packed_row_stride(n_columns);
    DevBuf<uint8_t> dpacked, dout;  // (device allocations are aligned far beyond the 16 bytes the kernels ask for)
    HIPCHK(c, dpacked.alloc(std::max<size_t>(bytes, 64)));
    if (bytes) HIPCHK(c, hipMemcpyAsync(dpacked.p, packed, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, dout.alloc((size_t)n_samples * (size_t)out_stride));
    if (int rc = region_states_on_device(c, dpacked.p, n_samples, n_sites, row_stride_bytes, site_begin, site_end, n_windows, src,
                                         n_columns, lo_num, hi_num, den, min_kept, region_long_sites(long_sites), dout.p,
                                         out_stride, nullptr))
      return rc;
    if (int rc = to_host(c, out_packed, dout)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ABN_OK;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

// ------------------------------------------------------------------------------------------------
// abn_regions_*: the getters of a region matrix
// ------------------------------------------------------------------------------------------------
extern "C" int abn_regions_destroy(abn_regions* h) { return handle_destroy(h); }

extern "C" int abn_regions_info(const abn_regions* h, int32_t* n_samples, int64_t* n_columns, int64_t* row_stride_bytes,
                                int32_t* n_groups) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (n_samples) *n_samples = h->n;
  if (n_columns) *n_columns = h->columns;
  if (row_stride_bytes) *row_stride_bytes = h->stride;
  if (n_groups) *n_groups = (int32_t)h->group_begin.size();
  return ABN_OK;
}

extern "C" int abn_regions_layout(const abn_regions* h, int64_t* group_begin, int64_t* group_end) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (group_begin) std::copy(h->group_begin.begin(), h->group_begin.end(), group_begin);
  if (group_end) std::copy(h->group_end.begin(), h->group_end.end(), group_end);
  return ABN_OK;
}

extern "C" int abn_regions_order(const abn_regions* h, int32_t* src) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (src) std::copy(h->src.begin(), h->src.end(), src);
  return ABN_OK;
}

extern "C" int abn_regions_packed(abn_regions* h, uint8_t* host_out) { return handle_packed(h, host_out); }

extern "C" int abn_regions_packed_device_ptr(abn_regions* h, void** dev_ptr) {
  if (!h || !dev_ptr) return ABN_ERR_INVALID_ARG;
  *dev_ptr = h->packed.p;
  return ABN_OK;
}

extern "C" int abn_regions_census(abn_regions* h, uint64_t* counts) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  const size_t G = h->group_begin.size();
  if (G == 0) return ABN_OK;
  if (!counts) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    DevBuf<unsigned long long> dcounts;
    HIPCHK(c, dcounts.alloc(G * (size_t)h->n * 3));
    if (int rc = packed_census_windows_dev(c, h->packed.p, h->n, h->columns, h->stride, h->group_begin.data(),
                                           h->group_end.data(), (int32_t)G, dcounts.p, nullptr))
      return rc;
    if (int rc = to_host(c, counts, dcounts)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ABN_OK;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_regions_pairwise(abn_regions* h, uint64_t* diff, uint64_t* both, double* dvalue) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  const size_t n = (size_t)h->n, npairs = n * (n - 1) / 2, G = h->group_begin.size();
  if (npairs == 0 || G == 0) return ABN_OK;
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    return pairwise_to_host(c, G * npairs, diff, both, dvalue, [&](auto* dd, auto* db, auto* dv) {
      return pairwise_windows_packed_dev(c, h->packed.p, h->n, h->columns, h->stride, h->group_begin.data(),
                                         h->group_end.data(), (int32_t)G, dd, db, dv, nullptr);
    });
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_regions_transitions(abn_regions* h, uint64_t* table) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  const size_t G = h->group_begin.size();
  if (h->n < 2 || G == 0) return ABN_OK;
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    return transitions_windows_packed_to_host(c, h->packed.p, h->n, h->columns, h->stride, h->group_begin.data(),
                                              h->group_end.data(), (int32_t)G, table);
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_regions_kernel_ms(const abn_regions* h, double* ms2) {
  if (!h || !ms2) return ABN_ERR_INVALID_ARG;
  std::copy(h->ms, h->ms + 2, ms2);
  return ABN_OK;
}
