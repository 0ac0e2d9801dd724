// Host-side infrastructure shared by the translation units of libabneutral_hip.so (the fit path's abn_api.hip,
// abn_context.hip and abn_plan.hip, which share abn_fit_host.hpp on top of this; abn_pairwise.hip, abn_windows.hip,
// abn_analyze.hip, abn_sites.hip, abn_genes.hip, abn_codes.hip, abn_sites_common.hip, abn_sites_union.hip, abn_tiles.hip,
// abn_resident.hip, abn_blocks.hip, abn_sites_sort.hip, abn_sites_dedup.hip, abn_sim.hip, abn_regions.hip): the context, its device-buffer pool, error reporting, the kernel_ms timer and the timing
// events of a call, the copies on the context's stream (upload, to_device, to_host), the shell of the windows, codes and
// tiles handles (created, destroyed, their packed matrix read), and what the consumers of resident methylomes share
// (abn_resident.hip).  Not part of the C-ABI (include/abneutral.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/abneutral.h"
#include "abn_sites_common.hpp"
#include "abn_sites_dedup.hpp"
#include "abn_sites_sort.hpp"
#include "abn_sites_union.hpp"

// ------------------------------------------------------------------------------------------------
// Device-buffer pool of a context.  The drop-in entry points (abn_ab_neutral_run, abn_boot_model_run, abn_cost_batch,
// abn_fit_batch: one call per window in the reference's loops) build and drop a plan per call — seventeen hipMalloc /
// hipFree pairs, several hundred microseconds next to a 1-3 ms fit.  Freed buffers of up to kPoolBufMax bytes are kept
// (at most kPoolTotalMax in all) and handed out again, best fit within 2x; everything is stream-ordered on the
// context's stream, and abn_shutdown frees the pool.
constexpr size_t kPoolBufMax = (size_t)64 << 20, kPoolTotalMax = (size_t)256 << 20;
struct BufPool {
  std::vector<std::pair<void*, size_t>> free_list;
  size_t held = 0;
  bool closed = false;  // abn_shutdown has run: buffers of plans that outlive their context are freed, not pooled
  void* take(size_t bytes, size_t* cap) {
    size_t best = free_list.size();
    for (size_t i = 0; i < free_list.size(); ++i)
      if (free_list[i].second >= bytes && free_list[i].second <= 2 * bytes + 256 &&
          (best == free_list.size() || free_list[i].second < free_list[best].second))
        best = i;
    if (best == free_list.size()) return nullptr;
    void* p = free_list[best].first;
    *cap = free_list[best].second;
    held -= *cap;
    free_list[best] = free_list.back();
    free_list.pop_back();
    return p;
  }
  bool give(void* p, size_t cap) {
    if (closed || cap > kPoolBufMax || held + cap > kPoolTotalMax) return false;
    free_list.emplace_back(p, cap);
    held += cap;
    return true;
  }
  void clear() {
    for (auto& e : free_list) (void)hipFree(e.first);
    free_list.clear();
    held = 0;
  }
};

struct abn_ctx {
  int device = -1;
  // read from hipDeviceProp at abn_init (MI355X: 256 CUs, 160 KiB of LDS per CU); every launch geometry below is a
  // multiple of the CU count, so a partitioned device (fewer CUs per logical GPU) gets proportionally smaller launches
  int cus = 256;
  size_t lds_per_cu = 160 * 1024;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::vector<hipStream_t> side;  // lazily created: window groups of a plan run concurrently on these
  // shared with every DevBuf drawn from it: a plan destroyed after abn_shutdown (easy from Python: ctx.close() before
  // the Plan is collected) still finds its pool — closed, so its buffers are simply freed
  std::shared_ptr<BufPool> pool = std::make_shared<BufPool>();
  std::string err;
};

// the pool DevBuf allocations of the current call draw from (set by PoolScope around the entry points)
inline thread_local std::shared_ptr<BufPool> g_pool;
struct PoolScope {
  std::shared_ptr<BufPool> prev;
  explicit PoolScope(abn_ctx* c) : prev(g_pool) { g_pool = c ? c->pool : nullptr; }
  ~PoolScope() { g_pool = prev; }
};

inline int set_err(abn_ctx* c, int status, const std::string& msg) {
  if (c) c->err = msg;
  return status;
}

#define HIPCHK(ctx, call)                                                                        \
  do {                                                                                           \
    hipError_t e__ = (call);                                                                     \
    if (e__ != hipSuccess)                                                                       \
      return set_err((ctx), ABN_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__));    \
  } while (0)

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  size_t cap = 0;          // bytes of the allocation behind p
  std::shared_ptr<BufPool> pool;  // where it came from / goes back to
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p && !(pool && pool->give(p, cap))) (void)hipFree(p);
    p = nullptr;
    n = 0;
    cap = 0;
  }
  hipError_t alloc(size_t count) {
    release();
    if (count == 0) return hipSuccess;
    const size_t bytes = count * sizeof(T);
    pool = g_pool;
    if (pool) {
      if (void* q = pool->take(bytes, &cap)) {
        p = (T*)q;
        n = count;
        return hipSuccess;
      }
    }
    hipError_t e = hipMalloc((void**)&p, bytes);
    if (e == hipErrorOutOfMemory && pool && pool->held) {  // the pool may be holding what this allocation needs
      (void)hipGetLastError();
      pool->clear();
      e = hipMalloc((void**)&p, bytes);
    }
    if (e == hipSuccess) {
      n = count;
      cap = bytes;
    }
    return e;
  }
  size_t bytes() const { return n * sizeof(T); }
};

// N timing events of one call, destroyed on every way out; span k runs from event k to event k + 1.  Where a call's
// kernel_ms is optional and one span is enough, EventPair below creates its events only when the time is wanted.
template <int N>
class Events {
 public:
  hipEvent_t e[N] = {};
  Events() = default;
  Events(const Events&) = delete;
  Events& operator=(const Events&) = delete;
  ~Events() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  int create(abn_ctx* c) {
    for (hipEvent_t& x : e)
      if (!x) HIPCHK(c, hipEventCreate(&x));
    return ABN_OK;
  }
  int record(abn_ctx* c, int k) {
    HIPCHK(c, hipEventRecord(e[k], c->stream));
    return ABN_OK;
  }
  // after a synchronisation behind event k + 1
  int elapsed_ms(abn_ctx* c, int k, double* ms) {
    float f = 0.f;
    HIPCHK(c, hipEventElapsedTime(&f, e[k], e[k + 1]));
    *ms = f;
    return ABN_OK;
  }
};

// The two HIP events around a call's kernels (kernel_ms): created when the time is first wanted, destroyed on every way
// out.
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  EventPair() = default;
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  ~EventPair() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  // in front of the kernels; nothing where the time is not wanted
  int begin(abn_ctx* c, bool wanted) {
    if (!wanted) return ABN_OK;
    if (!e0) HIPCHK(c, hipEventCreate(&e0));
    if (!e1) HIPCHK(c, hipEventCreate(&e1));
    HIPCHK(c, hipEventRecord(e0, c->stream));
    return ABN_OK;
  }
  // behind them: waits for the kernels and writes the milliseconds since begin; nothing for a null kernel_ms
  int end(abn_ctx* c, double* kernel_ms) {
    if (!kernel_ms) return ABN_OK;
    HIPCHK(c, hipEventRecord(e1, c->stream));
    HIPCHK(c, hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
    *kernel_ms = ms;
    return ABN_OK;
  }
};

// The tail of a host entry of the pairwise scans: the three outputs on the device — only those the caller wants; the
// scans take null outputs — around scan(ddiff, dboth, ddvalue), then to the host, and the stream synchronised.
template <class Scan>
int pairwise_to_host(abn_ctx* c, size_t count, uint64_t* diff, uint64_t* both, double* dvalue, Scan scan) {
  DevBuf<unsigned long long> ddiff, dboth;
  DevBuf<double> ddv;
  if (diff) HIPCHK(c, ddiff.alloc(count));
  if (both) HIPCHK(c, dboth.alloc(count));
  if (dvalue) HIPCHK(c, ddv.alloc(count));
  if (int rc = scan(ddiff.p, dboth.p, ddv.p)) return rc;
  if (diff) HIPCHK(c, hipMemcpyAsync(diff, ddiff.p, ddiff.bytes(), hipMemcpyDeviceToHost, c->stream));
  if (both) HIPCHK(c, hipMemcpyAsync(both, dboth.p, dboth.bytes(), hipMemcpyDeviceToHost, c->stream));
  if (dvalue) HIPCHK(c, hipMemcpyAsync(dvalue, ddv.p, ddv.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}

// The shell of the handles that hold a packed matrix — abn_windows, abn_codes, abn_tiles; each has `ctx` and `n` (samples)
// — behind their entry points' own checks.  handle_create: a handle of context c and n_samples samples around
// build(handle), on c's device and drawing from its pool; handed out in *out when build returns ABN_OK, else deleted.
// (abn_genes_create draws from no pool and abn_sites has a host form without a context: they keep their own.)
template <class H, class Build>
int handle_create(abn_ctx* c, int32_t n_samples, H** out, Build build) {
  std::unique_ptr<H> h(new (std::nothrow) H);
  if (!h) return set_err(c, ABN_ERR_HIP, "out of host memory");
  h->ctx = c;
  h->n = n_samples;
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    if (int rc = build(h.get())) return rc;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
  *out = h.release();
  return ABN_OK;
}
template <class H>
int handle_destroy(H* h) {
  if (!h) return ABN_ERR_INVALID_ARG;
  (void)hipSetDevice(h->ctx->device);
  delete h;
  return ABN_OK;
}
// ... and `packed` of an abn_windows or abn_codes to the host, the stream synchronised
template <class H>
int handle_packed(H* h, uint8_t* host_out) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  if (!host_out) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(host_out, h->packed.p, h->packed.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}

// The region matrix of a tiles handle (abn_tiles_region_states makes it in abn_tiles.hip, abn_regions.hip reads it): n
// rows of `stride` bytes, `columns` region fields each, the columns grouped into contiguous ranges
struct abn_regions {
  abn_ctx* ctx = nullptr;
  int n = 0;
  long long columns = 0, stride = 0;  // stride: abn_packed_row_stride(columns), at least 64
  DevBuf<uint8_t> packed;
  std::vector<int64_t> group_begin, group_end;  // [G] column ranges
  std::vector<int32_t> src;                     // [columns] the tile of each column
  double ms[2] = {0.0, 0.0};                    // the long tiles' census, the kernel
};

namespace abn {
// The copies on the context's stream, nothing waited for.  upload: `count` elements allocated and sent up from the host
template <class T>
int upload(abn_ctx* c, DevBuf<T>& buf, const T* host, size_t count) {
  HIPCHK(c, buf.alloc(count));
  HIPCHK(c, hipMemcpyAsync(buf.p, host, buf.bytes(), hipMemcpyHostToDevice, c->stream));
  return ABN_OK;
}
// ... to_device: `bytes` sent up into a buffer that stands
inline int to_device(abn_ctx* c, void* dst, const void* src, size_t bytes) {
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  return ABN_OK;
}
// ... and to_host: `bytes` from the device to dst; a null dst (an output the caller does not want) copies nothing
inline int to_host(abn_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!dst) return ABN_OK;
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  return ABN_OK;
}
template <class T>
int to_host(abn_ctx* c, void* dst, const DevBuf<T>& src) {
  return to_host(c, dst, src.p, src.bytes());
}

// abn_analyze.hip, for abn_plan_analyze (abn_plan.hip): the analysis (abn_analyze.hpp) of a device-resident table
// raw[W x B x 7] on the context's stream, results to the host; returns after completion, ABN_ERR_NO_FINITE_FIT as
// abn_analyze_batch.
int analyze_device_table(abn_ctx* c, const double* draw, int32_t W, int64_t B, double* out, int32_t* first_bad);
// abn_pairwise.hip, for abn_windows_pairwise (abn_windows.hip): abn_pairwise_divergence_windows_packed_dev behind its
// null check of the context.
int pairwise_windows_packed_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                                int32_t n_windows, void* dev_diff, void* dev_both, void* dev_dvalue, double* kernel_ms);
// ... and for abn_codes_transitions (abn_codes.hip) and abn_tiles_transitions (abn_tiles.hip): the entries
// abn_pairwise_transitions_packed_dev and _windows_packed_dev behind their null check of the context, and the windows
// one with its table [n_windows][pairs][9] copied to the host (n_samples >= 2 and n_windows >= 1; stream synchronised)
int transitions_packed_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                           int64_t row_stride_bytes, void* dev_table, double* kernel_ms);
int transitions_windows_packed_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                   int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                                   int32_t n_windows, void* dev_table, double* kernel_ms);
int transitions_windows_packed_to_host(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                                       int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                                       int32_t n_windows, uint64_t* table);
// ... and for abn_sim_study (abn_sim.hip): abn_packed_census_windows_dev behind its null check of the context
int packed_census_windows_dev(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites,
                              int64_t row_stride_bytes, const int64_t* site_begin, const int64_t* site_end,
                              int32_t n_windows, void* dev_counts, double* kernel_ms);
// abn_regions.hip, for abn_tiles_region_states (abn_tiles.hip): the region states (abn_regions.hpp) of a DEVICE matrix
// behind the checks of abn_packed_region_states_dev — HOST window and src arrays (src may be null: the identity), the rule
// valid, long_sites > 0 — into dev_out [n x out_stride]; ms2 (may be null): the long windows' census and the kernel.
// Returns after completion.
int region_states_on_device(abn_ctx* c, const void* dev_packed, int32_t n_samples, int64_t n_sites, int64_t row_stride_bytes,
                            const int64_t* site_begin, const int64_t* site_end, int64_t n_windows, const int32_t* src,
                            int64_t n_columns, int64_t lo_num, int64_t hi_num, int64_t den, int64_t min_kept, int64_t long_sites,
                            void* dev_out, int64_t out_stride, double* ms2);
// abn_blocks.hip, for abn_tiles_block_bootstrap (abn_tiles.hip): the block bootstrap (abn_blocks.hpp) of DEVICE tables —
// both, diff [n_blocks x n_pairs], level_sum_kept, kept [n_samples x n_blocks] — behind the checks of the groups: the counts
// of n_replicates + 1 rows per group made on the device, the sums of every row to the HOST outputs (any may be null), ms5 =
// the HIP-event times of counts, digits, product, finish and levels.  Returns after completion.
int blocks_bootstrap_dev(abn_ctx* c, uint64_t seed, int64_t n_groups, const uint32_t* group_id, const int64_t* group_begin,
                         const int64_t* group_end, int64_t n_replicates, int64_t n_blocks, int64_t n_pairs, int32_t n_samples,
                         const void* dev_both, const void* dev_diff, const double* dev_level_sum_kept, const int64_t* dev_kept,
                         uint64_t* both_out, uint64_t* diff_out, double* dvalue_out, double* level_out, int64_t* kept_out,
                         double* ms5);
// abn_genes.hip, for abn_windows_create_sites (abn_windows.hip): abn_genes_choose_dev behind its checks of the
// arguments, and the context a genes handle belongs to.
int genes_choose_dev(abn_genes* h, const abn_gene_rule* rule, int32_t n_samples, const int64_t* site_offset,
                     const int32_t* dchrom, const uint32_t* dstart, const uint32_t* dend, const uint8_t* dstrand,
                     uint32_t* dgene_start, uint32_t* dgene_end, uint8_t* dflags, double* kernel_ms);
abn_ctx* genes_ctx(const abn_genes* h);
// abn_sites.hip, for the builders from resident parse results (through abn_resident.hip, below).  The context of a
// resident handle (null: host form); its sites once the inserted records are in (-1: host form, or deferred lines without
// abn_sites_insert); and the merge (abn_sites_merge.hpp) of one sample into the arrays at its first site, on the context's
// stream, nothing waited for: the fields kernel of every chunk (inserted = false) or the insert kernel (true).
abn_ctx* sites_ctx(const abn_sites* h);
int64_t sites_merged_count(const abn_sites* h);
int sites_merge_dev(const abn_sites* h, bool inserted, double filter, int32_t* dchrom, uint32_t* dstart, uint32_t* dend,
                    uint8_t* dstrand, uint8_t* dcode, double* dlevel);
// ... and for abn_codes_create_parsed (abn_codes.hip): the same merge in its reduced form (abn_codes.hpp), the merged byte
// and the level of every site
int sites_merge_codes_dev(const abn_sites* h, bool inserted, double filter, uint8_t* dcode, double* dlevel);
// abn_sites.hip, for abn_sites_sort.hip: abn_parse_scan_kernel with a workgroup per row — the n counts at data + r * stride
// scanned in place (exclusive), their sum at entry n — for rows r = 0 .. rows - 1; nothing waited for
int sites_scan_rows(abn_ctx* c, uint32_t* data, uint32_t rows, uint32_t n, uint32_t stride);
// abn_sites_sort.hip, for abn_sites_sort (abn_sites.hip), all on the context's stream.  The flatten of one chunk's records
// and of the inserted records (dcontext: their context codes) into `out`, nothing waited for; sort_flat_dev: the check and
// the passes over the n flattened records, dorder [n] the permutation, info4 as abn_sites_sort_info, ms2 the HIP-event ms
// of the check and of the passes — returns after completion; the gather of the n records at dorder into `out`, nothing
// waited for
int sort_flatten_records_dev(abn_ctx* c, const MergeChunk& chunk, const long long* dinserted_line, long long n_inserted,
                             const SortFlat& out);
int sort_flatten_inserted_dev(abn_ctx* c, const MergeChunk* dchunks, const MergeInserted& ins, const uint8_t* dcontext,
                              const SortFlat& out);
int sort_flat_dev(abn_ctx* c, long long n, const SortFlat& flat, uint32_t* dorder, int64_t* info4, double* ms2);
int sort_gather_dev(abn_ctx* c, const SortFlat& in, const uint32_t* dorder, long long n, const ParseRecords& out);
// abn_sites_dedup.hip, for abn_sites_dedup (abn_sites.hip), on the context's stream.  dedup_flat_dev: the flags and the
// compaction over the n flattened records under `policy`, dorder (room for n) the kept records' indices, info4 as
// abn_sites_dedup_info, ms2 the HIP-event ms of the flags and of the compaction — returns after completion; the gather of
// the `kept` records at dorder, of n_in, into `out`, nothing waited for
int dedup_flat_dev(abn_ctx* c, long long n, const SortFlat& flat, int policy, uint32_t* dorder, int64_t* info4, double* ms2);
int dedup_gather_dev(abn_ctx* c, const SortFlat& in, const uint32_t* dorder, long long kept, long long n_in,
                     const ParseRecords& out);
// abn_codes.hip, for abn_tiles.hip too: the pack of n samples' merged bytes (sample s: dcode + dcode_off[s], a multiple of
// 16; dsite_off[s + 1] - dsite_off[s] sites) into dpacked [n x 4 row_dwords bytes]
int codes_pack_dev(abn_ctx* c, const uint8_t* dcode, const long long* dcode_off, const long long* dsite_off, int n,
                   long long row_dwords, uint8_t* dpacked);
// ... and the two offset arrays it reads, [n + 1] each: the host's, filled by the builder, and upload's copies of them on
// the device (nothing waited for: the host's stay until the stream has been)
struct PackOffsets {
  std::vector<int64_t> site, code;
  DevBuf<long long> dsite, dcode;
  int upload(abn_ctx* c) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the offsets on the device");
    HIPCHK(c, dsite.alloc(site.size()));
    HIPCHK(c, dcode.alloc(code.size()));
    HIPCHK(c, hipMemcpyAsync(dsite.p, site.data(), dsite.bytes(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dcode.p, code.data(), dcode.bytes(), hipMemcpyHostToDevice, c->stream));
    return ABN_OK;
  }
  void release() { site.clear(), code.clear(), dsite.release(), dcode.release(); }
};
// The checks every entry point makes of a site_offset [n_samples + 1] it is given
inline int site_offset_check(abn_ctx* c, int32_t n_samples, const int64_t* site_offset) {
  if (site_offset[0] != 0) return set_err(c, ABN_ERR_INVALID_ARG, "site_offset[0] is not 0");
  for (int s = 0; s < n_samples; ++s)
    if (site_offset[s + 1] < site_offset[s] || site_offset[s + 1] - site_offset[s] > 0xffffffffLL)
      return set_err(c, ABN_ERR_INVALID_ARG, "site_offset is not ascending, or a sample of 2^32 sites or more");
  return ABN_OK;
}
// abn_sites_common.hip: the run tables of the order checks (abn_sites_common.hpp) — per sample and chromosome key the first
// site of its run and the end of it — with the samples' offsets on the device and the err entries the checks leave.  The
// common-site step and the union step make them of their samples, abn_tiles.hip of its columns as one sample, whose tables
// stay with the handle.  set takes the offsets (host only: nothing is allocated); init allocates, fills (0x7f bytes:
// kCommonNone; run_end 0) and sends the offsets up; launch is the runs and ends passes over the sites (none: no launch);
// refusal reads err back, waits for the stream, and gives the first of the entries first .. last that is set (kind 0:
// none).
struct RunTables {
  int n = 0;
  std::vector<long long> site_off;  // [n + 1]
  DevBuf<long long> dsite_off, run_begin, run_end, err;
  long long sites() const { return site_off[(size_t)n]; }
  void set(int n_samples, const int64_t* site_offset);
  int init(abn_ctx* c);
  int launch(abn_ctx* c, const CommonSites& in);
  int refusal(abn_ctx* c, int first, int last, CommonRefusal* r);
};
// abn_sites_common.hip, for abn_windows_create_aligned and abn_codes_create_aligned: the common-site step
// (abn_sites_common.hpp) on DEVICE key arrays, in its two halves.  sites_common_match runs the order checks, the match and
// the ranks, waits, and leaves n_common in the state (dkeep [site_offset[n]], or null: the state's own); the caller sizes
// its aligned arrays and sites_common_gather fills them (any output of g may be null) and makes the co-ordering check.
// Either refuses with ABN_ERR_INVALID_ARG and the text of common_refusal_text.  Both return after completion.
struct CommonState {
  int probe = 0;
  long long Lp = 0, n_common = 0;
  CommonSites in{};
  uint8_t* keep = nullptr;
  DevBuf<uint8_t> keep_own;
  RunTables tab;
  DevBuf<uint32_t> match, src, block;
  Events<6> ev;
  double ms[4] = {0.0, 0.0, 0.0, 0.0};  // runs and ends; match; scan and rank; gather
};
int sites_common_match(abn_ctx* c, int n, const int64_t* site_offset, const CommonSites& in, uint8_t* dkeep, CommonState& st);
int sites_common_gather(abn_ctx* c, CommonState& st, const CommonGather& g);
// ... and the launch abn_sites_union.hip shares with it beside the run tables': the one-workgroup exclusive scan of
// data[0 .. n) with the sum at data[n]
int sites_common_scan(abn_ctx* c, uint32_t* data, uint32_t n);
// ... and what abn_sites_common* and abn_sites_union* check of their arguments (`out`: keep or dest; `count`: n_common or
// n_union)
int sites_keys_check(abn_ctx* c, int32_t n_samples, const int64_t* site_offset, const void* chromosome, const void* start,
                     const void* end, const void* strand, const void* out, const void* count);
// abn_sites_union.hip, for abn_windows_create_union and abn_codes_create_union: the union step (abn_sites_union.hpp) on
// DEVICE key arrays, in two halves as the common-site step.  sites_union_rank runs the order checks and every pass up to
// dest, waits in between for the refusals and n_union, and leaves n_union in the state (ddest [site_offset[n]], or null:
// the state's own); the caller sizes its arrays of n x n_union sites and sites_union_gather fills them (any output of g
// may be null).  sites_union_rank refuses with ABN_ERR_INVALID_ARG and the text of union_refusal_text.  Both return after
// completion.
struct UnionState {
  long long n_union = 0;
  CommonSites in{};
  uint32_t* dest = nullptr;
  RunTables tab;
  DevBuf<uint32_t> dest_own, owner, P, r, block, count, base, inv, own_at;
  DevBuf<int> order;
  Events<11> ev;  // 0..3 around the passes in front of the host's read, 4..7 around those behind it, 8..10 around the gather's
  double ms[kUnionPasses] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // runs and ends; owner; scan; base; rank; dest; invert; gather
};
int sites_union_rank(abn_ctx* c, int n, const int64_t* site_offset, const CommonSites& in, uint32_t* ddest, UnionState& st);
int sites_union_gather(abn_ctx* c, UnionState& st, const CommonGather& g);

// ------------------------------------------------------------------------------------------------
// abn_resident.hip: what the builders of handles from RESIDENT parse results share — windows_build_parsed
// (abn_windows.hip), codes_build (abn_codes.hip) and tiles_build (abn_tiles.hip).  Each is a prologue (the handles'
// refusals, the merge), an optional alignment, its gather, and the part that is the builder's own.
// ------------------------------------------------------------------------------------------------
// Every sample's sites (sites_merged_count) into counts [n_samples]; refuses, in this order per sample, a null handle, one
// in the host form, one of another context, one with deferred lines and no abn_sites_insert
int resident_counts(abn_ctx* c, int32_t n_samples, abn_sites* const* samples, int64_t* counts);
// The four key arrays of S sites on the device: allocated, or allocated and sent up from the host's (nothing waited for)
struct SiteKeys {
  DevBuf<int32_t> chrom;
  DevBuf<uint32_t> start, end;
  DevBuf<uint8_t> strand;
  CommonSites keys() const { return CommonSites{chrom.p, start.p, end.p, strand.p}; }
  int alloc(abn_ctx* c, size_t S);
  int upload(abn_ctx* c, size_t S, const int32_t* chromosome, const uint32_t* start_, const uint32_t* end_,
             const uint8_t* strand_);
};
// Where the reduced merge writes: sample s's merged bytes at code + code_off[s], its levels at level + level_off[s]
struct CodeTargets {
  uint8_t* code;
  const int64_t* code_off;
  double* level;
  const int64_t* level_off;
};
// The merged arrays of the first n_keyed samples, one sample behind the other from off[s] (at least one element each, so
// that no pointer is null).  merge_keyed is the full merge (sites_merge_dev) of those samples, keys included; merge_codes
// the reduced one (sites_merge_codes_dev) of n samples — `before`: their sites; a sample without any is skipped — into
// `to`, or (null) into code and level here, which takes n_keyed = n.  Both launch every sample's fields kernels, then the
// insert kernels, and wait for nothing; with `marks`, marks[0] and marks[1] are recorded in front of the two passes, and
// merge_keyed records marks[2] behind them.
struct MergedSites : SiteKeys {
  DevBuf<uint8_t> code;
  DevBuf<double> level;
  std::vector<int64_t> off;  // [n_keyed + 1]
  int alloc(abn_ctx* c, int n_keyed, const int64_t* count);
  int merge_keyed(abn_ctx* c, abn_sites* const* samples, double filter, const hipEvent_t* marks);
  int merge_codes(abn_ctx* c, int n, abn_sites* const* samples, const int64_t* before, double filter, const CodeTargets* to,
                  const hipEvent_t* marks);
};
// The alignment of n samples' merged arrays in front of a build: the mode (kAlignPosition or kAlignUnion) and the state of
// its step.  sites_align is sites_common_match or sites_union_rank and leaves `each`, the sites every sample has behind
// the step (n_common or n_union); the caller sizes its arrays of n x each sites and sites_align_gather fills them
// (sites_common_gather or sites_union_gather).  Refusals and completion as those.
struct Alignment {
  int mode = kAlignNone;
  int64_t each = 0;
  CommonState common;
  UnionState unite;
};
int sites_align(abn_ctx* c, int mode, int n, const int64_t* site_offset, const CommonSites& keys, Alignment& a);
int sites_align_gather(abn_ctx* c, Alignment& a, const CommonGather& g);
// What a handle reports of its alignment (abn_windows_common / _union, abn_codes_common / _union): every sample's sites as
// they came, and of the step that ran its count (-1: it did not run) and the HIP-event ms of its passes (after the gather)
struct AlignReport {
  std::vector<int64_t> before;  // [n]
  int64_t n_common = -1;        // ..._create_aligned: the sites every sample keeps
  double common_ms[4] = {0.0, 0.0, 0.0, 0.0};
  int64_t n_union = -1;         // ..._create_union: the sites every sample has, placeholders included
  double union_ms[kUnionPasses] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int common(int64_t* before_out, int64_t* n_common_out, double* ms4) const {
    if (before_out) std::copy(before.begin(), before.end(), before_out);
    if (n_common_out) *n_common_out = n_common;
    if (ms4) std::copy(common_ms, common_ms + 4, ms4);
    return ABN_OK;
  }
  int unite(int64_t* before_out, int64_t* n_union_out, double* ms8) const {
    if (before_out) std::copy(before.begin(), before.end(), before_out);
    if (n_union_out) *n_union_out = n_union;
    if (ms8) std::copy(union_ms, union_ms + kUnionPasses, ms8);
    return ABN_OK;
  }
};
void sites_align_report(const Alignment& a, AlignReport& r);
}  // namespace abn
