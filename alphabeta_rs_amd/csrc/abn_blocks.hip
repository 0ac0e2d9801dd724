// abn_block_*: the block bootstrap's counts and sums (abn_blocks.hpp: the definition, the kernels, the serial forms).
// One BlockRun is one call's launch chain on the context's stream — counts, digits, product, finish, levels, each between
// two events — and the one read of what the kernels flag; abn_tiles_block_bootstrap (abn_tiles.hip) runs the same chain
// behind its scan and folds through blocks_bootstrap_dev.
#include "abn_host.hpp"
#define ABN_BLOCKS_KERNELS
#include "abn_blocks.hpp"

using namespace abn;

namespace {

struct BlockTables {  // on the device: both, diff [T x P], level_sum_kept, kept [n x T]
  const unsigned long long *both, *diff;
  const double* level_sum_kept;
  const long long* kept;
};
struct BlockOutputs {  // on the device, any may be null: [G x rows x P] and [G x rows x n]
  unsigned long long *both, *diff;
  double *dvalue, *level;
  long long* kept;
};

struct BlockRun {
  abn_ctx* c = nullptr;
  long long G = 0, rows = 0, T = 0, P = 0, n = 0;
  std::vector<long long> gb, ge;
  DevBuf<long long> dgb, dge;
  DevBuf<uint32_t> dgid;
  DevBuf<BlockMeta> meta;
  DevBuf<uint8_t> planes;
  DevBuf<unsigned long long> both_own, diff_own;
  DevBuf<double> level_by_block;  // the two sample tables as [T][n], for the levels kernel
  DevBuf<long long> kept_by_block;
  BlockMeta flagged{};
  Events<6> ev;  // counts, digits, product, finish, levels
  double ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  bool drew = true;  // the counts kernel ran

  // the shape is valid (block_shape_refusal); G > 0
  int init(abn_ctx* ctx, long long n_groups, const int64_t* group_begin, const int64_t* group_end, long long rows_per_group,
           long long n_blocks, long long n_pairs, long long n_samples) {
    c = ctx;
    G = n_groups, rows = rows_per_group, T = n_blocks, P = n_pairs, n = n_samples;
    gb.assign(group_begin, group_begin + G), ge.assign(group_end, group_end + G);
    if (int rc = upload(c, dgb, gb.data(), (size_t)G)) return rc;
    if (int rc = upload(c, dge, ge.data(), (size_t)G)) return rc;
    HIPCHK(c, meta.alloc(1));
    HIPCHK(c, hipMemsetAsync(meta.p, 0, sizeof(BlockMeta), c->stream));
    if (int rc = ev.create(c)) return rc;
    return ev.record(c, 0);
  }

  // counts [G x rows x T] of rows - 1 replicates and the identity row; then event 1
  int counts(uint64_t seed, const uint32_t* group_id, uint8_t* dcounts) {
    if (int rc = upload(c, dgid, group_id, (size_t)G)) return rc;
    HIPCHK(c, hipMemsetAsync(dcounts, 0, (size_t)(G * rows) * (size_t)T, c->stream));
    long long longest = 0;
    for (long long g = 0; g < G; ++g) longest = std::max(longest, ge[(size_t)g] - gb[(size_t)g]);
    if (longest > 0) {
      const dim3 grid((unsigned)rows, (unsigned)G, (unsigned)((longest + kBlockHist - 1) / kBlockHist));
      hipLaunchKernelGGL(abn_block_counts_kernel, grid, dim3(kBlockThreads), 0, c->stream, seed, (const uint32_t*)dgid.p,
                         (const long long*)dgb.p, (const long long*)dge.p, (int)(rows - 1), T, dcounts, meta.p);
      HIPCHK(c, hipGetLastError());
    }
    return ev.record(c, 1);
  }
  int no_counts() {  // explicit counts: the span of the counts is reported as 0
    drew = false;
    return ev.record(c, 1);
  }

  // digits, product, finish, levels of explicit counts; planes_per_table: the digits the planes are sized for
  int resample(const uint8_t* dcounts, const BlockTables& t, BlockOutputs o, int planes_per_table) {
    const long long Tpad = block_padded_blocks(T), Ppad = block_padded_pairs(P);
    const long long values = G * rows * P;
    const bool product = values > 0 && (o.both || o.diff || o.dvalue);
    const long long row_jobs = (rows + 16 * kBlockRowTiles - 1) / (16 * kBlockRowTiles), col_jobs = (Ppad / 16 + 3) / 4;
    if (product && row_jobs * col_jobs >= kBlockJobsMax)
      return set_err(c, ABN_ERR_INVALID_ARG, "too many rows x pairs for one launch of the block product");
    if (product) {
      if (!o.both) {
        HIPCHK(c, both_own.alloc((size_t)values));
        o.both = both_own.p;
      }
      if (!o.diff) {
        HIPCHK(c, diff_own.alloc((size_t)values));
        o.diff = diff_own.p;
      }
      HIPCHK(c, planes.alloc((size_t)(2 * planes_per_table) * (size_t)Ppad * (size_t)Tpad));
      if (T > 0) {
        hipLaunchKernelGGL(abn_block_largest_kernel, dim3(block_grid((T * P + 7) / 8)), dim3(kBlockThreads), 0, c->stream, t.both,
                           t.diff, T * P, meta.p);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(abn_block_digits_kernel, dim3((unsigned)(Tpad / 64), (unsigned)(Ppad / 16)), dim3(kBlockThreads), 0,
                           c->stream, t.both, t.diff, T, P, Tpad, Ppad, planes_per_table, (const BlockMeta*)meta.p, planes.p);
        HIPCHK(c, hipGetLastError());
      }
    }
    if (int rc = ev.record(c, 2)) return rc;
    if (product) {
      BlockGemmArgs a{};
      a.counts = dcounts, a.planes = planes.p, a.group_begin = dgb.p, a.group_end = dge.p, a.meta = meta.p;
      a.both_out = o.both, a.diff_out = o.diff;
      a.n_blocks = T, a.n_pairs = P, a.Tpad = Tpad, a.Ppad = Ppad;
      a.rows = (int)rows, a.planes_per_table = planes_per_table, a.row_jobs = (int)row_jobs, a.col_jobs = (int)col_jobs;
      hipLaunchKernelGGL(abn_block_gemm_kernel, dim3((unsigned)(row_jobs * col_jobs), (unsigned)G), dim3(kBlockThreads), 0,
                         c->stream, a);
      HIPCHK(c, hipGetLastError());
    }
    if (int rc = ev.record(c, 3)) return rc;
    if (product && o.dvalue) {
      hipLaunchKernelGGL(abn_block_finish_kernel, dim3(block_grid(values)), dim3(kBlockThreads), 0, c->stream,
                         (const unsigned long long*)o.both, (const unsigned long long*)o.diff, values, o.dvalue);
      HIPCHK(c, hipGetLastError());
    }
    if (int rc = ev.record(c, 4)) return rc;
    if (G * rows * n > 0 && (o.level || o.kept)) {
      if (T > 0) {
        HIPCHK(c, level_by_block.alloc((size_t)(T * n)));
        HIPCHK(c, kept_by_block.alloc((size_t)(T * n)));
        hipLaunchKernelGGL(abn_block_transpose_kernel, dim3(block_grid(T * n)), dim3(kBlockThreads), 0, c->stream, t.level_sum_kept,
                           t.kept, T, (int)n, level_by_block.p, kept_by_block.p);
        HIPCHK(c, hipGetLastError());
      }
      hipLaunchKernelGGL(abn_block_levels_kernel, dim3(block_grid(G * rows * n)), dim3(kBlockThreads), 0, c->stream, dcounts,
                         (const long long*)dgb.p, (const long long*)dge.p, (int)G, (int)rows, T, (int)n,
                         (const double*)level_by_block.p, (const long long*)kept_by_block.p, o.level, o.kept);
      HIPCHK(c, hipGetLastError());
    }
    return ev.record(c, 5);
  }

  // what the kernels flagged to the host, the wait for the stream, the spans; the refusals of a flag
  int finish() {
    HIPCHK(c, hipMemcpyAsync(&flagged, meta.p, sizeof flagged, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 5; ++k)
      if (int rc = ev.elapsed_ms(c, k, &ms[k])) return rc;
    if (!drew) ms[0] = 0.0;
    if (flagged.over_value) return set_err(c, ABN_ERR_INVALID_ARG, "a table value of 2^35 or more");
    if (flagged.over_count) return set_err(c, ABN_ERR_INVALID_ARG, "a block count above 127");
    return ABN_OK;
  }
};

int refused(abn_ctx* c, const std::string& text) { return set_err(c, ABN_ERR_INVALID_ARG, text); }

// a host output's device twin: allocated only where the host wants the output
template <class T>
int twin(abn_ctx* c, DevBuf<T>& buf, const void* host, size_t count, T** dev) {
  *dev = nullptr;
  if (!host || count == 0) return ABN_OK;
  HIPCHK(c, buf.alloc(count));
  *dev = buf.p;
  return ABN_OK;
}

struct HostOutputs {  // the five outputs of an entry with host buffers, their device twins, and the copies back
  DevBuf<unsigned long long> both, diff;
  DevBuf<double> dvalue, level;
  DevBuf<long long> kept;
  BlockOutputs dev{};
  int alloc(abn_ctx* c, size_t pair_values, size_t sample_values, const uint64_t* both_out, const uint64_t* diff_out,
            const double* dvalue_out, const double* level_out, const int64_t* kept_out) {
    if (int rc = twin(c, both, both_out, pair_values, &dev.both)) return rc;
    if (int rc = twin(c, diff, diff_out, pair_values, &dev.diff)) return rc;
    if (int rc = twin(c, dvalue, dvalue_out, pair_values, &dev.dvalue)) return rc;
    if (int rc = twin(c, level, level_out, sample_values, &dev.level)) return rc;
    return twin(c, kept, kept_out, sample_values, &dev.kept);
  }
  int to_host_all(abn_ctx* c, uint64_t* both_out, uint64_t* diff_out, double* dvalue_out, double* level_out, int64_t* kept_out) {
    if (dev.both) if (int rc = to_host(c, both_out, both)) return rc;
    if (dev.diff) if (int rc = to_host(c, diff_out, diff)) return rc;
    if (dev.dvalue) if (int rc = to_host(c, dvalue_out, dvalue)) return rc;
    if (dev.level) if (int rc = to_host(c, level_out, level)) return rc;
    if (dev.kept) if (int rc = to_host(c, kept_out, kept)) return rc;
    return ABN_OK;
  }
};

}  // namespace

namespace abn {
int blocks_bootstrap_dev(abn_ctx* c, uint64_t seed, int64_t n_groups, const uint32_t* group_id, const int64_t* group_begin,
                         const int64_t* group_end, int64_t n_replicates, int64_t n_blocks, int64_t n_pairs, int32_t n_samples,
                         const void* dev_both, const void* dev_diff, const double* dev_level_sum_kept, const int64_t* dev_kept,
                         uint64_t* both_out, uint64_t* diff_out, double* dvalue_out, double* level_out, int64_t* kept_out,
                         double* ms5) {
  if (n_replicates < 0) return refused(c, "a negative size");
  const long long rows = n_replicates + 1;
  const std::string why = block_shape_refusal(n_groups, group_begin, group_end, rows, n_blocks);
  if (!why.empty()) return refused(c, why);
  if (n_groups > 0 && !group_id) return refused(c, "null/size");
  if (ms5) std::fill(ms5, ms5 + 5, 0.0);
  if (n_groups == 0) return ABN_OK;
  try {
  BlockRun run;
  HostOutputs out;
  DevBuf<uint8_t> dcounts;
  if (int rc = run.init(c, n_groups, group_begin, group_end, rows, n_blocks, n_pairs, n_samples)) return rc;
  HIPCHK(c, dcounts.alloc(std::max<size_t>((size_t)(n_groups * rows) * (size_t)n_blocks, 1)));
  if (int rc = out.alloc(c, (size_t)(n_groups * rows * n_pairs), (size_t)(n_groups * rows * n_samples), both_out, diff_out,
                         dvalue_out, level_out, kept_out))
    return rc;
  if (int rc = run.counts(seed, group_id, dcounts.p)) return rc;
  const BlockTables t{(const unsigned long long*)dev_both, (const unsigned long long*)dev_diff, dev_level_sum_kept,
                      (const long long*)dev_kept};
  if (int rc = run.resample(dcounts.p, t, out.dev, kBlockDigitsMax)) return rc;
  if (int rc = out.to_host_all(c, both_out, diff_out, dvalue_out, level_out, kept_out)) return rc;
  const int rc = run.finish();
  if (ms5) std::copy(run.ms, run.ms + 5, ms5);
  return rc;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}
}  // namespace abn

extern "C" int abn_block_counts(abn_ctx* c, uint64_t seed, int32_t n_groups, const uint32_t* group_id,
                                const int64_t* group_begin, const int64_t* group_end, int64_t n_replicates, int64_t n_blocks,
                                uint8_t* counts) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (n_replicates < 0) return refused(c, "a negative size");
  const long long rows = n_replicates + 1;
  const std::string why = block_shape_refusal(n_groups, group_begin, group_end, rows, n_blocks);
  if (!why.empty()) return refused(c, why);
  const size_t bytes = (size_t)(n_groups * rows) * (size_t)n_blocks;
  if (bytes == 0) return ABN_OK;
  if (!group_id || !counts) return refused(c, "null/size");
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    BlockRun run;
    DevBuf<uint8_t> dcounts;
    if (int rc = run.init(c, n_groups, group_begin, group_end, rows, n_blocks, 0, 0)) return rc;
    HIPCHK(c, dcounts.alloc(bytes));
    if (int rc = run.counts(seed, group_id, dcounts.p)) return rc;
    for (int k = 2; k < 6; ++k)
      if (int rc = run.ev.record(c, k)) return rc;
    if (int rc = to_host(c, counts, dcounts)) return rc;
    return run.finish();
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_block_counts_host(uint64_t seed, int32_t n_groups, const uint32_t* group_id, const int64_t* group_begin,
                                     const int64_t* group_end, int64_t n_replicates, int64_t n_blocks, uint8_t* counts,
                                     char* text, int32_t text_bytes) {
  auto say = [&](const std::string& s) {
    if (text && text_bytes > 0) snprintf(text, (size_t)text_bytes, "%s", s.c_str());
    return s.empty() ? ABN_OK : ABN_ERR_INVALID_ARG;
  };
  say("");
  if (n_replicates < 0) return say("a negative size");
  const std::string why = block_shape_refusal(n_groups, group_begin, group_end, n_replicates + 1, n_blocks);
  if (!why.empty()) return say(why);
  if ((size_t)(n_groups * (n_replicates + 1)) * (size_t)n_blocks == 0) return ABN_OK;
  if (!group_id || !counts) return say("null/size");
  try {
    if (!block_counts_host(seed, n_groups, group_id, group_begin, group_end, n_replicates, n_blocks, counts))
      return say("a block count above 127");
  } catch (const std::bad_alloc&) {
    return say("out of host memory");
  }
  return ABN_OK;
}

extern "C" int abn_block_resample_host(int32_t n_groups, const int64_t* group_begin, const int64_t* group_end,
                                       int64_t rows_per_group, const uint8_t* counts, int64_t n_blocks, int64_t n_pairs,
                                       int32_t n_samples, const uint64_t* both, const uint64_t* diff,
                                       const double* level_sum_kept, const int64_t* kept, uint64_t* both_out,
                                       uint64_t* diff_out, double* dvalue_out, double* level_out, int64_t* kept_out, char* text,
                                       int32_t text_bytes) {
  auto say = [&](const std::string& s) {
    if (text && text_bytes > 0) snprintf(text, (size_t)text_bytes, "%s", s.c_str());
    return s.empty() ? ABN_OK : ABN_ERR_INVALID_ARG;
  };
  say("");
  std::string why = block_shape_refusal(n_groups, group_begin, group_end, rows_per_group, n_blocks);
  if (why.empty()) why = block_tables_refusal(n_blocks, n_pairs, n_samples, both, diff, level_sum_kept, kept, nullptr);
  if (why.empty()) why = block_counts_refusal(n_groups, group_begin, group_end, rows_per_group, n_blocks, counts);
  if (!why.empty()) return say(why);
  try {
    block_resample_host(n_groups, group_begin, group_end, rows_per_group, counts, n_blocks, n_pairs, n_samples, both, diff,
                        level_sum_kept, kept, both_out, diff_out, dvalue_out, level_out, kept_out);
  } catch (const std::bad_alloc&) {
    return say("out of host memory");
  }
  return ABN_OK;
}

extern "C" int abn_block_resample(abn_ctx* c, int32_t n_groups, const int64_t* group_begin, const int64_t* group_end,
                                  int64_t rows_per_group, const uint8_t* counts, int64_t n_blocks, int64_t n_pairs,
                                  int32_t n_samples, const uint64_t* both, const uint64_t* diff, const double* level_sum_kept,
                                  const int64_t* kept, uint64_t* both_out, uint64_t* diff_out, double* dvalue_out,
                                  double* level_out, int64_t* kept_out) {
  if (!c) return ABN_ERR_INVALID_ARG;
  uint64_t largest = 0;
  std::string why = block_shape_refusal(n_groups, group_begin, group_end, rows_per_group, n_blocks);
  if (why.empty()) why = block_tables_refusal(n_blocks, n_pairs, n_samples, both, diff, level_sum_kept, kept, &largest);
  if (why.empty()) why = block_counts_refusal(n_groups, group_begin, group_end, rows_per_group, n_blocks, counts);
  if (!why.empty()) return refused(c, why);
  const long long all_rows = (long long)n_groups * rows_per_group;
  if (all_rows == 0) return ABN_OK;
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    BlockRun run;
    HostOutputs out;
    DevBuf<uint8_t> dcounts;
    DevBuf<unsigned long long> dboth, ddiff;
    DevBuf<double> dlevel;
    DevBuf<long long> dkept;
    if (int rc = run.init(c, n_groups, group_begin, group_end, rows_per_group, n_blocks, n_pairs, n_samples)) return rc;
    if (int rc = run.no_counts()) return rc;
    const size_t cbytes = (size_t)all_rows * (size_t)n_blocks, tp = (size_t)(n_blocks * n_pairs), tn = (size_t)n_blocks * (size_t)n_samples;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t) && sizeof(long long) == sizeof(int64_t), "tables");
    if (cbytes) if (int rc = upload(c, dcounts, counts, cbytes)) return rc;
    if (tp) {
      if (int rc = upload(c, dboth, (const unsigned long long*)both, tp)) return rc;
      if (int rc = upload(c, ddiff, (const unsigned long long*)diff, tp)) return rc;
    }
    if (tn) {
      if (int rc = upload(c, dlevel, level_sum_kept, tn)) return rc;
      if (int rc = upload(c, dkept, (const long long*)kept, tn)) return rc;
    }
    if (int rc = out.alloc(c, (size_t)(all_rows * n_pairs), (size_t)all_rows * (size_t)n_samples, both_out, diff_out, dvalue_out,
                           level_out, kept_out))
      return rc;
    if (int rc = run.resample(dcounts.p, BlockTables{dboth.p, ddiff.p, dlevel.p, dkept.p}, out.dev, block_digits_of(largest)))
      return rc;
    if (int rc = out.to_host_all(c, both_out, diff_out, dvalue_out, level_out, kept_out)) return rc;
    return run.finish();
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_block_resample_dev(abn_ctx* c, int32_t n_groups, const int64_t* group_begin, const int64_t* group_end,
                                      int64_t rows_per_group, const void* dev_counts, int64_t n_blocks, int64_t n_pairs,
                                      int32_t n_samples, const void* dev_both, const void* dev_diff,
                                      const void* dev_level_sum_kept, const void* dev_kept, void* dev_both_out,
                                      void* dev_diff_out, void* dev_dvalue_out, void* dev_level_out, void* dev_kept_out,
                                      double* ms5) {
  if (!c) return ABN_ERR_INVALID_ARG;
  const std::string why = block_shape_refusal(n_groups, group_begin, group_end, rows_per_group, n_blocks);
  if (!why.empty()) return refused(c, why);
  if (n_pairs < 0 || n_samples < 0) return refused(c, "a negative size");
  const long long all_rows = (long long)n_groups * rows_per_group;
  if (ms5) std::fill(ms5, ms5 + 5, 0.0);
  if (all_rows == 0) return ABN_OK;
  if (n_blocks > 0 && (!dev_counts || (n_pairs > 0 && (!dev_both || !dev_diff)) ||
                       (n_samples > 0 && (!dev_level_sum_kept || !dev_kept))))
    return refused(c, "null/size");
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    BlockRun run;
    if (int rc = run.init(c, n_groups, group_begin, group_end, rows_per_group, n_blocks, n_pairs, n_samples)) return rc;
    if (int rc = run.no_counts()) return rc;
    const BlockTables t{(const unsigned long long*)dev_both, (const unsigned long long*)dev_diff,
                        (const double*)dev_level_sum_kept, (const long long*)dev_kept};
    const BlockOutputs o{(unsigned long long*)dev_both_out, (unsigned long long*)dev_diff_out, (double*)dev_dvalue_out,
                         (double*)dev_level_out, (long long*)dev_kept_out};
    if (int rc = run.resample((const uint8_t*)dev_counts, t, o, kBlockDigitsMax)) return rc;
    const int rc = run.finish();
    if (ms5) std::copy(run.ms, run.ms + 5, ms5);
    return rc;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}
