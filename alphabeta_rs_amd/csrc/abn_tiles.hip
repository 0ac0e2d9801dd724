// abn_tiles_*: genomic tiles over resident, aligned methylomes — Pedigree::build (src/pedigree.rs:147-172, :210-261) once
// per fixed bin or listed region.  Kernels, the definition and the serial forms: abn_tiles.hpp.  The build is
// abn_codes.hip's (merge, optional common-site or union step, gather, pack) with the columns' keys, the merged bytes and the
// levels kept; the front end both share is abn_resident.hip's, the handle's shell, the pack launch and its offsets
// (handle_create, codes_pack_dev, PackOffsets) abn_host.hpp's, the merge launches are abn_sites.hip's, the order checks
// (RunTables) abn_sites_common.hip's, the scan abn_pairwise.hip's.  The handle's own matrix and the pooled one are two
// TileMatrix records; the tiles run and the pools run are made of the same steps (interval upload, search, fold, results),
// the pools run with offsets, map, gather and pack in between.
#include "abn_host.hpp"
#define ABN_TILES_KERNELS
#include "abn_tiles.hpp"
#include "abn_regions.hpp"  // (the plain arithmetic: abn_tiles_region_states checks with it; the kernel is abn_regions.hip's)

using namespace abn;

// A uniform matrix, n rows of `columns` sites, as the pack writes it and the fold and the scan read it.  tiles_matrix_shape
// gives the strides — false: the matrix is beyond the limits of a handle (tiles_matrix_fits), and the caller refuses it
// with its own text; alloc takes the shape, allocates the three arrays and sends the pack's offsets up; pack is the
// launch, nothing waited for.
struct MatrixShape {
  long long columns = 0;
  long long stride = 0;       // bytes per row of `packed`
  long long code_stride = 0;  // bytes per sample of `code`: columns up to a multiple of 16
};

static bool tiles_matrix_shape(int n, long long columns, MatrixShape* shape) {
  *shape = MatrixShape{columns, std::max<long long>(abn_packed_row_stride(columns), 64),
                       (columns + 15) / 16 * 16};  // (whole 16-byte loads of the pack)
  return tiles_matrix_fits(n, columns, shape->stride);
}

struct TileMatrix : MatrixShape {
  DevBuf<uint8_t> packed;  // [n x stride]
  DevBuf<uint8_t> code;    // [n x code_stride] merged bytes
  DevBuf<double> level;    // [n x columns]
  PackOffsets off;         // sample s: its sites from s x columns, its merged bytes from s x code_stride

  int alloc(abn_ctx* c, int n, const MatrixShape& shape) {
    MatrixShape::operator=(shape);
    const size_t rows = (size_t)n;
    HIPCHK(c, code.alloc(std::max<size_t>(rows * (size_t)code_stride, 16)));
    HIPCHK(c, level.alloc(rows * std::max<size_t>((size_t)columns, 1)));
    HIPCHK(c, packed.alloc(rows * (size_t)stride));
    off.site.resize(rows + 1), off.code.resize(rows + 1);
    for (size_t s = 0; s <= rows; ++s) off.site[s] = (int64_t)s * columns, off.code[s] = (int64_t)s * code_stride;
    return off.upload(c);
  }
  int pack(abn_ctx* c, int n) { return codes_pack_dev(c, code.p, off.dcode.p, off.dsite.p, n, stride / 4, packed.p); }
  void release_staging() { code.release(), level.release(), off.release(); }  // what only a build reads: `packed` stays
  void reset() {
    MatrixShape::operator=(MatrixShape{});
    packed.release(), release_staging();
  }
};

struct abn_tiles {
  abn_ctx* ctx = nullptr;
  int n = 0;
  TileMatrix own;             // the handle's own matrix, whole
  DevBuf<int32_t> chromosome; // [own.columns] the columns' keys
  DevBuf<uint32_t> start;
  RunTables tables;           // of the columns as one sample: run_begin, run_end [kCommonChroms]
  std::vector<TileRun> runs;
  bool has_tiles = false;
  std::vector<int32_t> tchromosome;  // [T] the intervals
  std::vector<int64_t> tstart, tend;
  std::vector<int64_t> begin, end;   // [T] their columns
  std::vector<double> level_sum_kept;  // [n x T]
  std::vector<int64_t> kept;
  double ms[2] = {0.0, 0.0};  // search, fold
  // pools (abn_tiles_set_pools): the tiles are the pools, their columns those of the pooled matrix
  bool pooled = false;
  TileMatrix pool;             // the pooled matrix: `packed` alone outlives abn_tiles_set_pools
  DevBuf<long long> pool_src;  // [pool.columns] every pooled column's source column
  PoolSegments segments;
  std::vector<int64_t> seg_begin, seg_end;  // [S] the segments' columns
  double pool_ms[4] = {0.0, 0.0, 0.0, 0.0};  // offsets, map, gather, pack
  // the block bootstrap (abn_tiles_block_bootstrap): the tiles came from abn_tiles_set_fixed and do not overlap
  bool fixed_disjoint = false;
  double block_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // counts, digits, product, finish, levels of the last call

  void drop_pools() {
    pooled = false;
    pool.reset();
    pool_src.release();
    segments = PoolSegments{};
    seg_begin.clear();
    seg_end.clear();
    std::fill(pool_ms, pool_ms + 4, 0.0);
  }
};

static int tiles_build(abn_tiles* h, double filter, abn_sites* const* samples, int align,
                       const std::vector<int64_t>& before) {
  abn_ctx* c = h->ctx;
  const int n = h->n;
  // the prologue and the alignment.  The full merge, keys included: of every sample under an alignment, of sample 0 alone
  // without one
  MergedSites m;
  Alignment a;
  if (int rc = m.alloc(c, align ? n : 1, before.data())) return rc;
  if (int rc = m.merge_keyed(c, samples, filter, nullptr)) return rc;
  long long each = before[0];
  if (align) {
    if (int rc = sites_align(c, align, n, m.off.data(), m.keys(), a)) return rc;
    each = a.each;
  }
  TileMatrix& own = h->own;
  MatrixShape shape;
  if (!tiles_matrix_shape(n, each, &shape)) return set_err(c, ABN_ERR_INVALID_ARG, "packed matrix too large for one handle");
  if (int rc = own.alloc(c, n, shape)) return rc;
  const size_t E = std::max<size_t>((size_t)each, 1);
  HIPCHK(c, h->chromosome.alloc(E));
  HIPCHK(c, h->start.alloc(E));

  // the reduced merge: the merged bytes (merge_code has no kCodeCounted) and the levels, into the merged arrays under an
  // alignment, else straight into the handle's
  const CodeTargets kept{own.code.p, own.off.code.data(), own.level.p, own.off.site.data()};
  if (int rc = m.merge_codes(c, n, samples, before.data(), filter, align ? nullptr : &kept, nullptr)) return rc;
  // the columns' four key fields, for the order checks: sample 0's after the gather, or as merged
  SiteKeys gkey;
  CommonSites columns = m.keys();
  if (align) {
    if (int rc = gkey.alloc(c, (size_t)n * E)) return rc;
    const CommonGather g{m.code.p,      m.level.p,  gkey.chrom.p, gkey.start.p,  gkey.end.p,
                         gkey.strand.p, own.level.p, own.code.p,   own.code_stride};
    if (int rc = sites_align_gather(c, a, g)) return rc;
    columns = gkey.keys();  // (sample 0's are the first `each` of each)
  }
  // the builder's own: the columns' keys, their run tables and the pack
  if (each > 0) {
    HIPCHK(c, hipMemcpyAsync(h->chromosome.p, columns.chromosome, (size_t)each * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(h->start.p, columns.start, (size_t)each * 4, hipMemcpyDeviceToDevice, c->stream));
  }
  // the runs and ends passes over the columns as one sample: the run tables, and the order checks' refusals
  RunTables& tab = h->tables;
  const int64_t col_off[2] = {0, each};
  DevBuf<uint32_t> dlast;
  tab.set(1, col_off);
  if (int rc = tab.init(c)) return rc;
  HIPCHK(c, dlast.alloc(kCommonChroms));
  if (int rc = tab.launch(c, columns)) return rc;
  hipLaunchKernelGGL(abn_tiles_last_kernel, dim3((kCommonChroms + kTilesThreads - 1) / kTilesThreads), dim3(kTilesThreads), 0,
                     c->stream, (const uint32_t*)h->start.p, (const long long*)tab.run_begin.p,
                     (const long long*)tab.run_end.p, dlast.p);
  HIPCHK(c, hipGetLastError());
  if (int rc = own.pack(c, n)) return rc;

  long long run_begin[kCommonChroms], run_end[kCommonChroms];
  uint32_t last[kCommonChroms];
  CommonRefusal r;
  HIPCHK(c, hipMemcpyAsync(run_begin, tab.run_begin.p, sizeof run_begin, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(run_end, tab.run_end.p, sizeof run_end, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(last, dlast.p, sizeof last, hipMemcpyDeviceToHost, c->stream));
  if (int rc = tab.refusal(c, kCommonSplitRun, kCommonBadKey, &r)) return rc;  // (waits; the merged arrays are freed on return)
  tab.dsite_off.release();  // the handle keeps the two tables alone
  tab.err.release();
  own.off.release();  // the pack has read its offsets (code and level stay: the folds and the pools read them)
  if (r.kind)
    return set_err(c, ABN_ERR_INVALID_ARG,
                   "the sites cannot be cut into tiles: their keys are not well ordered: " + common_refusal_text(r));
  tiles_runs_from_tables(run_begin, run_end, last, &h->runs);
  return ABN_OK;
}

extern "C" int abn_tiles_create(abn_ctx* c, double posterior_max_filter, int32_t align, int32_t n_samples,
                                abn_sites* const* samples, abn_tiles** out) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (out) *out = nullptr;
  if (!out || !samples || n_samples <= 0) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n_samples > 65535) return set_err(c, ABN_ERR_INVALID_ARG, "too many samples");
  if (align != kAlignNone && align != kAlignPosition && align != kAlignUnion)
    return set_err(c, ABN_ERR_INVALID_ARG, "align expects 0 (none), 1 (position) or 2 (union)");
  return handle_create(c, n_samples, out, [&](abn_tiles* h) {
    std::vector<int64_t> count((size_t)n_samples, 0);
    if (int rc = resident_counts(c, n_samples, samples, count.data())) return rc;
    if (align == kAlignNone)
      for (int s = 1; s < n_samples; ++s)
        if (count[(size_t)s] != count[0])
          return set_err(c, ABN_ERR_INVALID_ARG,
                         "sample " + std::to_string(s) + " has " + std::to_string(count[(size_t)s]) + " sites, sample 0 has " +
                             std::to_string(count[0]) +
                             ": tiles need the same sites in every sample; align them with --align position or --align union");
    return tiles_build(h, posterior_max_filter, samples, align, count);
  });
}

extern "C" int abn_tiles_destroy(abn_tiles* h) { return handle_destroy(h); }

extern "C" int abn_tiles_info(const abn_tiles* h, int32_t* n_samples, int64_t* n_columns, int64_t* row_stride_bytes,
                              int32_t* n_runs, int64_t* n_tiles) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (n_samples) *n_samples = h->n;
  if (n_columns) *n_columns = h->own.columns;
  if (row_stride_bytes) *row_stride_bytes = h->own.stride;
  if (n_runs) *n_runs = (int32_t)h->runs.size();
  if (n_tiles) *n_tiles = h->has_tiles ? (int64_t)h->begin.size() : -1;
  return ABN_OK;
}

extern "C" int abn_tiles_runs(const abn_tiles* h, int32_t* chromosome, int64_t* first, int64_t* count, uint32_t* last_start) {
  if (!h) return ABN_ERR_INVALID_ARG;
  for (size_t r = 0; r < h->runs.size(); ++r) {
    if (chromosome) chromosome[r] = h->runs[r].chromosome;
    if (first) first[r] = h->runs[r].first;
    if (count) count[r] = h->runs[r].count;
    if (last_start) last_start[r] = h->runs[r].last_start;
  }
  return ABN_OK;
}

// ------------------------------------------------------------------------------------------------
// The steps the tiles run (tiles_run) and the pools run (tiles_run_pools) are made of, each on the context's stream; none
// waits, none records an event: the spans of kernel_ms and pool_kernel_ms are their callers'.
// ------------------------------------------------------------------------------------------------
// An interval list on the device (no interval: nothing is allocated, nothing sent)
struct DevIntervals {
  DevBuf<int32_t> chrom;
  DevBuf<long long> pos, pos_end;
  template <class Pos>
  int upload(abn_ctx* c, const std::vector<int32_t>& chromosome, const std::vector<Pos>& start, const std::vector<Pos>& end) {
    static_assert(sizeof(Pos) == sizeof(long long), "positions");
    const size_t count = chromosome.size();
    HIPCHK(c, chrom.alloc(count));
    HIPCHK(c, pos.alloc(count));
    HIPCHK(c, pos_end.alloc(count));
    if (count == 0) return ABN_OK;
    HIPCHK(c, hipMemcpyAsync(chrom.p, chromosome.data(), chrom.bytes(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(pos.p, start.data(), pos.bytes(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(pos_end.p, end.data(), pos_end.bytes(), hipMemcpyHostToDevice, c->stream));
    return ABN_OK;
  }
};

// The column ranges of T tiles and what the fold makes of them, [n x T], on the device
struct DevTiles {
  DevBuf<long long> begin, end, kept;
  DevBuf<double> sum;
  int alloc(abn_ctx* c, size_t n, size_t T) {
    HIPCHK(c, begin.alloc(T));
    HIPCHK(c, end.alloc(T));
    HIPCHK(c, sum.alloc(n * T));
    HIPCHK(c, kept.alloc(n * T));
    return ABN_OK;
  }
};

// the search of the intervals' columns in the handle's own matrix: [iv's count] begin, end (no interval: no launch)
static int tiles_search(const abn_tiles* h, const DevIntervals& iv, long long* begin, long long* end) {
  abn_ctx* c = h->ctx;
  const size_t count = iv.chrom.n;
  if (count == 0) return ABN_OK;
  hipLaunchKernelGGL(abn_tiles_search_kernel, dim3((unsigned)((count + kTilesThreads - 1) / kTilesThreads)), dim3(kTilesThreads),
                     0, c->stream, (const uint32_t*)h->start.p, (const long long*)h->tables.run_begin.p,
                     (const long long*)h->tables.run_end.p, (long long)count, (const int32_t*)iv.chrom.p,
                     (const long long*)iv.pos.p, (const long long*)iv.pos_end.p, begin, end);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

// the folds of every sample over the ranges r.begin, r.end [T > 0] of m's columns
static int tiles_fold(const abn_tiles* h, const TileMatrix& m, size_t T, DevTiles& r) {
  abn_ctx* c = h->ctx;
  hipLaunchKernelGGL(abn_tiles_fold_kernel, dim3((unsigned)T, (unsigned)h->n), dim3(kCodesWave), 0, c->stream,
                     (const uint8_t*)m.code.p, m.code_stride, (const double*)m.level.p, m.columns, (long long)T,
                     (const long long*)r.begin.p, (const long long*)r.end.p, r.sum.p, r.kept.p);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

// the results of T tiles: the handle's arrays sized, and (T > 0) the copies of r into them queued
static int tiles_results(abn_tiles* h, size_t T, const DevTiles& r) {
  abn_ctx* c = h->ctx;
  const size_t n = (size_t)h->n;
  h->begin.assign(T, 0);
  h->end.assign(T, 0);
  h->level_sum_kept.assign(n * T, 0.0);
  h->kept.assign(n * T, 0);
  if (T == 0) return ABN_OK;
  static_assert(sizeof(long long) == sizeof(int64_t), "columns");
  HIPCHK(c, hipMemcpyAsync(h->begin.data(), r.begin.p, r.begin.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(h->end.data(), r.end.p, r.end.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(h->level_sum_kept.data(), r.sum.p, r.sum.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(h->kept.data(), r.kept.p, r.kept.bytes(), hipMemcpyDeviceToHost, c->stream));
  return ABN_OK;
}

// the search and the folds of the handle's interval list; the list is valid
static int tiles_run(abn_tiles* h) {
  abn_ctx* c = h->ctx;
  const size_t T = h->tchromosome.size();
  h->ms[0] = h->ms[1] = 0.0;
  if (T == 0) return tiles_results(h, 0, DevTiles{});
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevIntervals iv;
  DevTiles r;
  if (int rc = iv.upload(c, h->tchromosome, h->tstart, h->tend)) return rc;
  if (int rc = r.alloc(c, (size_t)h->n, T)) return rc;
  Events<3> ev;
  if (int rc = ev.create(c)) return rc;
  if (int rc = ev.record(c, 0)) return rc;
  if (int rc = tiles_search(h, iv, r.begin.p, r.end.p)) return rc;
  if (int rc = ev.record(c, 1)) return rc;
  if (int rc = tiles_fold(h, h->own, T, r)) return rc;
  if (int rc = ev.record(c, 2)) return rc;
  if (int rc = tiles_results(h, T, r)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 2; ++k)
    if (int rc = ev.elapsed_ms(c, k, &h->ms[k])) return rc;
  return ABN_OK;
}

static int tiles_set(abn_tiles* h, std::vector<int32_t>& chromosome, std::vector<int64_t>& start, std::vector<int64_t>& end) {
  h->has_tiles = false;
  h->fixed_disjoint = false;
  (void)hipSetDevice(h->ctx->device);
  h->drop_pools();  // back on the handle's own matrix
  h->tchromosome.swap(chromosome);
  h->tstart.swap(start);
  h->tend.swap(end);
  const int rc = tiles_run(h);
  h->has_tiles = rc == ABN_OK;
  return rc;
}

// the refusal of the k-th of a list (`what`: "tile" or "interval") that tiles_interval_valid does not take
static int tiles_interval_refused(abn_ctx* c, const char* what, int64_t k) {
  return set_err(c, ABN_ERR_INVALID_ARG,
                 what + (" " + std::to_string(k)) + ": a chromosome outside 0..257, or a start or end outside [0, 2^32]");
}

extern "C" int abn_tiles_set_intervals(abn_tiles* h, int64_t n_tiles, const int32_t* chromosome, const int64_t* start,
                                       const int64_t* end) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  if (n_tiles < 0 || (n_tiles > 0 && (!chromosome || !start || !end))) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n_tiles > 0x7fffffffLL) return set_err(c, ABN_ERR_INVALID_ARG, "more tiles than INT32_MAX");
  for (int64_t t = 0; t < n_tiles; ++t)
    if (!tiles_interval_valid(chromosome[t], start[t], end[t])) return tiles_interval_refused(c, "tile", t);
  try {
    std::vector<int32_t> tc(chromosome, chromosome + n_tiles);
    std::vector<int64_t> ts(start, start + n_tiles), te(end, end + n_tiles);
    return tiles_set(h, tc, ts, te);
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_tiles_set_fixed(abn_tiles* h, int64_t size, int64_t step) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  if (size <= 0 || step < 0) return set_err(c, ABN_ERR_INVALID_ARG, "a tile size of 0 or less, or a step below 0");
  const long long T = tiles_fixed_intervals(h->runs.data(), (int)h->runs.size(), size, step, nullptr, nullptr, nullptr);
  if (T > 0x7fffffffLL) return set_err(c, ABN_ERR_INVALID_ARG, "more tiles than INT32_MAX");
  try {
    std::vector<int32_t> tc((size_t)T);
    std::vector<int64_t> ts((size_t)T), te((size_t)T);
    tiles_fixed_intervals(h->runs.data(), (int)h->runs.size(), size, step, tc.data(), (long long*)ts.data(),
                          (long long*)te.data());
    const int rc = tiles_set(h, tc, ts, te);
    h->fixed_disjoint = rc == ABN_OK && (step == 0 || step >= size);
    return rc;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

// The pools of a merged segment list (abn_tiles.hpp: pools), one launch chain on the context's stream: search, offsets and
// ranges; the read of the pooled total, the one wait inside the chain — the pooled arrays are sized from it, and a total
// beyond the limits of a handle's matrix is refused there, the handle untouched; then map, gather, pack and fold, and the
// wait for the results.  Behind the refusals the handle leaves what it held; a HIP error leaves it without tiles.
static int tiles_run_pools(abn_tiles* h, PoolSegments& seg, int32_t n_pools) {
  abn_ctx* c = h->ctx;
  const size_t S = seg.size(), P = (size_t)n_pools;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevIntervals iv;
  DevTiles r;  // of the pools
  DevBuf<long long> dcol_begin, dcol_end, dseg_off, dseg_first;
  if (int rc = iv.upload(c, seg.chromosome, seg.start, seg.end)) return rc;
  HIPCHK(c, dcol_begin.alloc(S));
  HIPCHK(c, dcol_end.alloc(S));
  HIPCHK(c, dseg_off.alloc(S + 1));
  HIPCHK(c, dseg_first.alloc(P + 1));
  if (int rc = r.alloc(c, (size_t)h->n, P)) return rc;
  HIPCHK(c, hipMemcpyAsync(dseg_first.p, seg.seg_first.data(), dseg_first.bytes(), hipMemcpyHostToDevice, c->stream));
  Events<8> ev;  // 0..2 around search and offsets, in front of the host's read; 3..7 around map, gather, pack and fold
  if (int rc = ev.create(c)) return rc;
  if (int rc = ev.record(c, 0)) return rc;
  if (int rc = tiles_search(h, iv, dcol_begin.p, dcol_end.p)) return rc;  // the segments' columns
  if (int rc = ev.record(c, 1)) return rc;
  hipLaunchKernelGGL(abn_tiles_pool_offsets_kernel, dim3(1), dim3(kTilesThreads), 0, c->stream, (const long long*)dcol_begin.p,
                     (const long long*)dcol_end.p, (long long)S, dseg_off.p);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(abn_tiles_pool_ranges_kernel, dim3((unsigned)((P + kTilesThreads - 1) / kTilesThreads)), dim3(kTilesThreads), 0,
                     c->stream, (const long long*)dseg_off.p, (const long long*)dseg_first.p, (long long)P, r.begin.p, r.end.p);
  HIPCHK(c, hipGetLastError());
  if (int rc = ev.record(c, 2)) return rc;
  long long pooled = 0;
  HIPCHK(c, hipMemcpyAsync(&pooled, dseg_off.p + S, sizeof pooled, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  MatrixShape shape;
  if (!tiles_matrix_shape(h->n, pooled, &shape))
    return set_err(c, ABN_ERR_INVALID_ARG,
                   "pooled matrix too large for one handle: " + std::to_string(pooled) + " pooled columns");

  // from here on the handle changes
  h->has_tiles = false;
  h->fixed_disjoint = false;
  h->drop_pools();
  h->tchromosome.clear(), h->tstart.clear(), h->tend.clear();
  const TileMatrix& own = h->own;
  TileMatrix& pm = h->pool;
  if (int rc = pm.alloc(c, h->n, shape)) return rc;
  HIPCHK(c, h->pool_src.alloc(std::max<size_t>((size_t)pooled, 1)));
  const dim3 columns((unsigned)((pooled + kTilesThreads - 1) / kTilesThreads), (unsigned)h->n);
  if (int rc = ev.record(c, 3)) return rc;
  if (pooled > 0) {
    hipLaunchKernelGGL(abn_tiles_pool_map_kernel, dim3(columns.x), dim3(kTilesThreads), 0, c->stream,
                       (const long long*)dseg_off.p, (long long)S, (const long long*)dcol_begin.p, pooled, h->pool_src.p);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = ev.record(c, 4)) return rc;
  if (pooled > 0) {
    hipLaunchKernelGGL(abn_tiles_pool_gather_kernel, columns, dim3(kTilesThreads), 0, c->stream, (const uint8_t*)own.code.p,
                       own.code_stride, (const double*)own.level.p, own.columns, (const long long*)h->pool_src.p, pooled,
                       pm.code.p, pm.code_stride, pm.level.p);
    HIPCHK(c, hipGetLastError());
  }
  if (int rc = ev.record(c, 5)) return rc;
  if (int rc = pm.pack(c, h->n)) return rc;
  if (int rc = ev.record(c, 6)) return rc;
  if (int rc = tiles_fold(h, pm, P, r)) return rc;
  if (int rc = ev.record(c, 7)) return rc;
  h->seg_begin.assign(S, 0), h->seg_end.assign(S, 0);
  static_assert(sizeof(long long) == sizeof(int64_t), "columns");
  if (S > 0) {
    HIPCHK(c, hipMemcpyAsync(h->seg_begin.data(), dcol_begin.p, dcol_begin.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h->seg_end.data(), dcol_end.p, dcol_end.bytes(), hipMemcpyDeviceToHost, c->stream));
  }
  if (int rc = tiles_results(h, P, r)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  pm.release_staging();  // the scan reads `packed` alone
  const int span[6] = {0, 6, 1, 3, 4, 5};  // search, fold; offsets, map, gather, pack
  for (int k = 0; k < 6; ++k)
    if (int rc = ev.elapsed_ms(c, span[k], k < 2 ? &h->ms[k] : &h->pool_ms[k - 2])) return rc;
  h->segments = std::move(seg);
  h->pooled = h->has_tiles = true;
  return ABN_OK;
}

extern "C" int abn_tiles_set_pools(abn_tiles* h, int64_t n_intervals, const int32_t* chromosome, const int64_t* start,
                                   const int64_t* end, const int32_t* pool, int64_t n_pools) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  if (n_intervals < 0 || (n_intervals > 0 && (!chromosome || !start || !end || !pool)))
    return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n_pools <= 0) return set_err(c, ABN_ERR_INVALID_ARG, "n_pools is 0 or less");
  if (n_pools > 0x7fffffffLL) return set_err(c, ABN_ERR_INVALID_ARG, "more pools than INT32_MAX");
  for (int64_t k = 0; k < n_intervals; ++k) {
    if (pool[k] < 0 || pool[k] >= n_pools)
      return set_err(c, ABN_ERR_INVALID_ARG,
                     "interval " + std::to_string(k) + ": pool " + std::to_string(pool[k]) + " outside 0.." +
                         std::to_string(n_pools - 1));
    if (!tiles_interval_valid(chromosome[k], start[k], end[k])) return tiles_interval_refused(c, "interval", k);
  }
  try {
    PoolSegments seg;
    tiles_pool_merge(h->runs.data(), (int)h->runs.size(), n_intervals, chromosome, (const long long*)start,
                     (const long long*)end, pool, (int32_t)n_pools, &seg);
    const int rc = tiles_run_pools(h, seg, (int32_t)n_pools);
    if (rc && !h->has_tiles) h->drop_pools();
    return rc;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_tiles_pool_segments(const abn_tiles* h, int64_t* n_segments, int32_t* pool, int32_t* chromosome,
                                       int64_t* start, int64_t* end, int64_t* col_begin, int64_t* col_end) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (!h->has_tiles || !h->pooled) return set_err(h->ctx, ABN_ERR_INVALID_ARG, "no pools: abn_tiles_set_pools first");
  const PoolSegments& s = h->segments;
  if (n_segments) *n_segments = (int64_t)s.size();
  if (pool) std::copy(s.pool.begin(), s.pool.end(), pool);
  if (chromosome) std::copy(s.chromosome.begin(), s.chromosome.end(), chromosome);
  if (start) std::copy(s.start.begin(), s.start.end(), start);
  if (end) std::copy(s.end.begin(), s.end.end(), end);
  if (col_begin) std::copy(h->seg_begin.begin(), h->seg_begin.end(), col_begin);
  if (col_end) std::copy(h->seg_end.begin(), h->seg_end.end(), col_end);
  return ABN_OK;
}

extern "C" int abn_tiles_pool_columns(const abn_tiles* h, int64_t* src) {
  if (!h) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = h->ctx;
  if (!h->has_tiles || !h->pooled) return set_err(c, ABN_ERR_INVALID_ARG, "no pools: abn_tiles_set_pools first");
  if (!src || h->pool.columns == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(src, h->pool_src.p, (size_t)h->pool.columns * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}

extern "C" int abn_tiles_pool_kernel_ms(const abn_tiles* h, double* ms4) {
  if (!h || !ms4) return ABN_ERR_INVALID_ARG;
  std::copy(h->pool_ms, h->pool_ms + 4, ms4);
  return ABN_OK;
}

static int tiles_need(const abn_tiles* h) {
  if (!h) return ABN_ERR_INVALID_ARG;
  if (!h->has_tiles) return set_err(h->ctx, ABN_ERR_INVALID_ARG, "no tiles yet: abn_tiles_set_intervals or abn_tiles_set_fixed first");
  return ABN_OK;
}

extern "C" int abn_tiles_intervals(const abn_tiles* h, int32_t* chromosome, int64_t* start, int64_t* end) {
  if (int rc = tiles_need(h)) return rc;
  if (h->pooled)
    return set_err(h->ctx, ABN_ERR_INVALID_ARG,
                   "the tiles are pools, each a set of segments and no one interval: abn_tiles_pool_segments gives them");
  if (chromosome) std::copy(h->tchromosome.begin(), h->tchromosome.end(), chromosome);
  if (start) std::copy(h->tstart.begin(), h->tstart.end(), start);
  if (end) std::copy(h->tend.begin(), h->tend.end(), end);
  return ABN_OK;
}

extern "C" int abn_tiles_layout(const abn_tiles* h, int64_t* begin, int64_t* end) {
  if (int rc = tiles_need(h)) return rc;
  if (begin) std::copy(h->begin.begin(), h->begin.end(), begin);
  if (end) std::copy(h->end.begin(), h->end.end(), end);
  return ABN_OK;
}

extern "C" int abn_tiles_stats(const abn_tiles* h, int64_t* count, double* level_sum_kept, int64_t* kept) {
  if (int rc = tiles_need(h)) return rc;
  if (count)
    for (size_t t = 0; t < h->begin.size(); ++t) count[t] = h->end[t] - h->begin[t];
  if (level_sum_kept) std::copy(h->level_sum_kept.begin(), h->level_sum_kept.end(), level_sum_kept);
  if (kept) std::copy(h->kept.begin(), h->kept.end(), kept);
  return ABN_OK;
}

extern "C" int abn_tiles_pairwise(abn_tiles* h, uint64_t* diff, uint64_t* both, double* dvalue) {
  if (int rc = tiles_need(h)) return rc;
  abn_ctx* c = h->ctx;
  const size_t n = (size_t)h->n, npairs = n * (n - 1) / 2, T = h->begin.size();
  if (npairs == 0 || T == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  const TileMatrix& m = h->pooled ? h->pool : h->own;
  return pairwise_to_host(c, T * npairs, diff, both, dvalue, [&](auto* dd, auto* db, auto* dv) {
    return pairwise_windows_packed_dev(c, m.packed.p, h->n, m.columns, m.stride, h->begin.data(), h->end.data(), (int32_t)T, dd,
                                       db, dv, nullptr);
  });
}

extern "C" int abn_tiles_transitions(abn_tiles* h, uint64_t* table) {
  if (int rc = tiles_need(h)) return rc;
  abn_ctx* c = h->ctx;
  const size_t T = h->begin.size();
  if (h->n < 2 || T == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  const TileMatrix& m = h->pooled ? h->pool : h->own;
  return transitions_windows_packed_to_host(c, m.packed.p, h->n, m.columns, m.stride, h->begin.data(), h->end.data(),
                                            (int32_t)T, table);
}

// The region matrix of the handle's tiles (abn_regions.hpp): every tile one column, called from the tile's sites of the
// handle's own matrix; the columns in ascending (group, tile), so that every group is one contiguous column range.  The new
// handle owns its matrix: nothing of `h` is kept.
extern "C" int abn_tiles_region_states(abn_tiles* h, int64_t lo_num, int64_t hi_num, int64_t den, int64_t min_kept,
                                       const int32_t* group, int32_t n_groups, abn_regions** out) {
  if (out) *out = nullptr;
  if (int rc = tiles_need(h)) return rc;
  abn_ctx* c = h->ctx;
  if (!out) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (h->pooled)
    return set_err(c, ABN_ERR_INVALID_ARG,
                   "the tiles are pools: a pool is a class of sites, not a region; abn_tiles_set_intervals or "
                   "abn_tiles_set_fixed first");
  if (n_groups < 1) return set_err(c, ABN_ERR_INVALID_ARG, "n_groups is below 1");
  const size_t T = h->begin.size(), G = (size_t)n_groups;
  try {
    // the columns: a counting sort of the tiles by group, stable, so ascending (group, tile)
    std::vector<int64_t> first(G + 1, 0);
    for (size_t t = 0; t < T; ++t) {
      const int32_t g = group ? group[t] : 0;
      if (g < -1 || g >= n_groups)
        return set_err(c, ABN_ERR_INVALID_ARG,
                       "tile " + std::to_string(t) + ": group " + std::to_string(g) + " outside -1.." + std::to_string(n_groups - 1));
      if (g >= 0) ++first[(size_t)g + 1];
    }
    for (size_t g = 0; g < G; ++g) first[g + 1] += first[g];
    const int64_t C = first[G];
    std::vector<int32_t> src((size_t)C);
    std::vector<int64_t> at(first.begin(), first.end() - 1);
    for (size_t t = 0; t < T; ++t) {
      const int32_t g = group ? group[t] : 0;
      if (g >= 0) src[(size_t)at[(size_t)g]++] = (int32_t)t;
    }
    const TileMatrix& m = h->own;
    const int32_t none = 0;  // every tile left out: C = 0, an empty matrix and no error — src is then no null pointer either
    const int32_t* columns = C > 0 ? src.data() : &none;
    const std::string why = region_refusal(m.packed.p, h->n, m.columns, m.stride, h->begin.data(), h->end.data(), (int64_t)T,
                                           columns, C, lo_num, hi_num, den, min_kept, 0, m.packed.p);
    if (!why.empty()) return set_err(c, ABN_ERR_INVALID_ARG, why);
    return handle_create(c, h->n, out, [&](abn_regions* r) {
      r->columns = C;
      r->stride = std::max<long long>(abn_packed_row_stride(C), 64);
      HIPCHK(c, r->packed.alloc((size_t)h->n * (size_t)r->stride));
      if (C == 0) HIPCHK(c, hipMemsetAsync(r->packed.p, 0xff, r->packed.bytes(), c->stream));  // one step of filtered fields
      if (int rc = region_states_on_device(c, m.packed.p, h->n, m.columns, m.stride, h->begin.data(), h->end.data(), (int64_t)T,
                                           columns, C, lo_num, hi_num, den, min_kept, region_long_sites(0), r->packed.p,
                                           r->stride, r->ms))
        return rc;
      HIPCHK(c, hipStreamSynchronize(c->stream));
      r->group_begin.assign(first.begin(), first.end() - 1);
      r->group_end.assign(first.begin() + 1, first.end());
      r->src.swap(src);
      return (int)ABN_OK;
    });
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_tiles_kernel_ms(const abn_tiles* h, double* ms2) {
  if (!h || !ms2) return ABN_ERR_INVALID_ARG;
  std::copy(h->ms, h->ms + 2, ms2);
  return ABN_OK;
}

// The groups abn_tiles_block_bootstrap draws in, in block space: every pool's segments, or the one group of all tiles
extern "C" int abn_tiles_block_groups(const abn_tiles* h, int64_t* n_groups, int64_t* n_blocks, int64_t* group_begin,
                                      int64_t* group_end) {
  if (int rc = tiles_need(h)) return rc;
  const size_t G = h->pooled ? h->begin.size() : 1, S = h->pooled ? h->seg_begin.size() : h->begin.size();
  if (n_groups) *n_groups = (int64_t)G;
  if (n_blocks) *n_blocks = (int64_t)S;
  for (size_t g = 0; g < G; ++g) {
    if (group_begin) group_begin[g] = h->pooled ? (int64_t)h->segments.seg_first[g] : 0;
    if (group_end) group_end[g] = h->pooled ? (int64_t)h->segments.seg_first[g + 1] : (int64_t)S;
  }
  return ABN_OK;
}

// The block bootstrap of the handle's tiles (abn_blocks.hpp).  The blocks are the pools' merged segments in segment order,
// one group per pool, or the fixed tiles in one group; their tables come from the windows scan and the fold over the
// handle's OWN matrix at the blocks' columns, stay on the device, and go straight into the counts, digits, product, finish
// and levels chain of blocks_bootstrap_dev: between the scan and the outputs only the flags of the chain cross to the host.
extern "C" int abn_tiles_block_bootstrap(abn_tiles* h, uint64_t seed, int64_t n_replicates, uint64_t* both_out,
                                         uint64_t* diff_out, double* dvalue_out, double* level_out, int64_t* kept_out) {
  if (int rc = tiles_need(h)) return rc;
  abn_ctx* c = h->ctx;
  if (!h->pooled && !h->fixed_disjoint)
    return set_err(c, ABN_ERR_INVALID_ARG,
                   "the tiles may overlap: the block bootstrap takes pools (abn_tiles_set_pools) or fixed tiles whose step is 0 "
                   "or at least their size (abn_tiles_set_fixed)");
  try {
    const std::vector<int64_t>& bb = h->pooled ? h->seg_begin : h->begin;
    const std::vector<int64_t>& be = h->pooled ? h->seg_end : h->end;
    const size_t S = bb.size(), n = (size_t)h->n, P = n * (n - 1) / 2;
    if (S > 0x7fffffffULL) return set_err(c, ABN_ERR_INVALID_ARG, "more blocks than INT32_MAX");
    int64_t G = 0;
    abn_tiles_block_groups(h, &G, nullptr, nullptr, nullptr);
    std::vector<uint32_t> gid((size_t)G, 0u);
    std::vector<int64_t> gb((size_t)G, 0), ge((size_t)G, 0);
    abn_tiles_block_groups(h, nullptr, nullptr, gb.data(), ge.data());
    for (size_t g = 0; g < gid.size(); ++g) gid[g] = (uint32_t)g;  // group_id = pool (fixed tiles: the one group 0)
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    DevTiles r;
    DevBuf<unsigned long long> ddiff, dboth;
    if (S > 0) {
      if (int rc = r.alloc(c, n, S)) return rc;
      if (int rc = to_device(c, r.begin.p, bb.data(), r.begin.bytes())) return rc;
      if (int rc = to_device(c, r.end.p, be.data(), r.end.bytes())) return rc;
      if (int rc = tiles_fold(h, h->own, S, r)) return rc;
      if (P > 0) {
        HIPCHK(c, ddiff.alloc(S * P));
        HIPCHK(c, dboth.alloc(S * P));
        if (int rc = pairwise_windows_packed_dev(c, h->own.packed.p, h->n, h->own.columns, h->own.stride, bb.data(), be.data(),
                                                 (int32_t)S, ddiff.p, dboth.p, nullptr, nullptr))
          return rc;
      }
    }
    return blocks_bootstrap_dev(c, seed, (int64_t)gid.size(), gid.data(), gb.data(), ge.data(), n_replicates, (int64_t)S,
                                (int64_t)P, h->n, dboth.p, ddiff.p, r.sum.p, (const int64_t*)r.kept.p, both_out, diff_out,
                                dvalue_out, level_out, kept_out, h->block_ms);
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_tiles_block_ms(const abn_tiles* h, double* ms5) {
  if (!h || !ms5) return ABN_ERR_INVALID_ARG;
  std::copy(h->block_ms, h->block_ms + 5, ms5);
  return ABN_OK;
}
