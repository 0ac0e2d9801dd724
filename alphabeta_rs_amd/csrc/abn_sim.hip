// abn_sim_*: methylomes simulated down a pedigree under the ABneutral model (abn_sim.hpp: the law, the thresholds, the
// kernel, the serial forms).  One launch on the context's stream between two events; abn_sim_pedigree runs the two packed
// scans (abn_pairwise.hip: the divergence, the transition table) on the simulated matrix where it lies.  abn_sim_observe*
// is the observation step (miscalls and dropouts) over a packed matrix; abn_sim_study simulates R replicates as the column
// ranges of one matrix, observes them in place, and scans and counts all of them in one windows scan and one census.
#include "abn_host.hpp"
#define ABN_SIM_KERNELS
#include "abn_sim.hpp"

using namespace abn;

namespace {

int refused(abn_ctx* c, const std::string& text) { return set_err(c, ABN_ERR_INVALID_ARG, text); }

// The launch of valid arguments into dout [n_emit x stride] on the device (L > 0); returns after completion
int sim_run(abn_ctx* c, uint64_t seed, int32_t V, const int32_t* parent, const uint64_t* thr, const uint8_t* emit, int64_t L,
            uint8_t* dout, int64_t stride, double* kernel_ms) {
  const SimPlan plan = sim_plan(V, parent, emit);
  const int64_t row_bytes = sim_row_bytes(L), row_dwords = row_bytes / 4;
  DevBuf<SimNode> dnodes;
  DevBuf<uint64_t> dthr;
  DevBuf<uint8_t> dscratch;
  EventPair ev;
  double ms = 0.0;
  if (int rc = upload(c, dnodes, plan.nodes.data(), (size_t)V)) return rc;
  if (int rc = upload(c, dthr, thr, (size_t)V * 6)) return rc;
  HIPCHK(c, dscratch.alloc((size_t)plan.n_scratch * (size_t)row_bytes));
  const unsigned blocks = (unsigned)sim_grid_blocks(row_dwords, c->cus);
  bool lazy = true;
#ifdef ABN_MEASUREMENT_KNOBS  // scripts/simulate_ab.py: the variant that always draws the low words
  if (const char* e = getenv("ABN_SIM_BOTH")) lazy = atoi(e) == 0;
#endif
  if (int rc = ev.begin(c, true)) return rc;
  if (lazy)
    hipLaunchKernelGGL(abn_sim_codes_kernel<true>, dim3(blocks), dim3(kSimThreads), 0, c->stream, seed, V, (const SimNode*)dnodes.p,
                       (const uint64_t*)dthr.p, L, row_dwords, dout, stride, dscratch.p, row_bytes);
  else
    hipLaunchKernelGGL(abn_sim_codes_kernel<false>, dim3(blocks), dim3(kSimThreads), 0, c->stream, seed, V, (const SimNode*)dnodes.p,
                       (const uint64_t*)dthr.p, L, row_dwords, dout, stride, dscratch.p, row_bytes);
  HIPCHK(c, hipGetLastError());
  if (int rc = ev.end(c, &ms)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (kernel_ms) *kernel_ms = ms;
  return ABN_OK;
}

// The observation of valid arguments on device matrices (L > 0); returns after completion
int observe_run(abn_ctx* c, uint64_t seed, int32_t n_rows, const int32_t* node_of_row, const uint64_t* othr, int64_t L,
                const uint8_t* din, int64_t in_stride, uint8_t* dout, int64_t out_stride, double* kernel_ms) {
  const int64_t row_dwords = sim_row_bytes(L) / 4;
  DevBuf<int32_t> dnodes;
  EventPair ev;
  double ms = 0.0;
  if (int rc = upload(c, dnodes, node_of_row, (size_t)n_rows)) return rc;
  const ObsThr t = sim_obs_thr(othr);
  const dim3 grid((unsigned)sim_grid_blocks(row_dwords, c->cus), (unsigned)n_rows);
  bool lazy = true;
#ifdef ABN_MEASUREMENT_KNOBS  // the variant that always draws the low words, switched as the simulation's is
  if (const char* e = getenv("ABN_SIM_BOTH")) lazy = atoi(e) == 0;
#endif
  if (int rc = ev.begin(c, true)) return rc;
  if (lazy)
    hipLaunchKernelGGL(abn_sim_observe_kernel<true>, grid, dim3(kSimThreads), 0, c->stream, seed, (const int32_t*)dnodes.p, t, L,
                       row_dwords, din, in_stride, dout, out_stride);
  else
    hipLaunchKernelGGL(abn_sim_observe_kernel<false>, grid, dim3(kSimThreads), 0, c->stream, seed, (const int32_t*)dnodes.p, t, L,
                       row_dwords, din, in_stride, dout, out_stride);
  HIPCHK(c, hipGetLastError());
  if (int rc = ev.end(c, &ms)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (kernel_ms) *kernel_ms = ms;
  return ABN_OK;
}

}  // namespace

extern "C" int abn_sim_thresholds(double alpha, double beta, double p_uu0, double weight, int32_t n_nodes, const int32_t* parent,
                                  const int32_t* generation, uint64_t* thr, char* text, int32_t text_bytes) {
  std::string why;
  try {
    why = sim_thresholds(alpha, beta, p_uu0, weight, n_nodes, parent, generation, thr);
  } catch (const std::bad_alloc&) {
    why = "out of host memory";
  }
  if (text && text_bytes > 0) snprintf(text, (size_t)text_bytes, "%s", why.c_str());
  return why.empty() ? ABN_OK : ABN_ERR_INVALID_ARG;
}

extern "C" int abn_sim_grid(abn_ctx* c, int64_t n_sites, int32_t* grid2) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (!grid2 || n_sites < 0 || n_sites > kSimMaxSites) return refused(c, "null/size");
  grid2[0] = n_sites == 0 ? 0 : (int32_t)sim_grid_blocks(sim_row_bytes(n_sites) / 4, c->cus);
  grid2[1] = kSimThreads;
  return ABN_OK;
}

extern "C" int abn_sim_codes_dev(abn_ctx* c, uint64_t seed, int32_t n_nodes, const int32_t* parent, const uint64_t* thr,
                                 const uint8_t* emit, int64_t n_sites, void* dev_packed, int64_t row_stride_bytes,
                                 double* kernel_ms) {
  if (!c) return ABN_ERR_INVALID_ARG;
  const std::string why = sim_refusal(n_nodes, parent, thr, emit, n_sites, dev_packed, row_stride_bytes);
  if (!why.empty()) return refused(c, why);
  if (((uintptr_t)dev_packed & 15u) != 0) return refused(c, "abn_sim_codes_dev: dev_packed is not 16-byte aligned");
  if (kernel_ms) *kernel_ms = 0.0;
  if (n_sites == 0) return ABN_OK;
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    return sim_run(c, seed, n_nodes, parent, thr, emit, n_sites, (uint8_t*)dev_packed, row_stride_bytes, kernel_ms);
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_sim_codes(abn_ctx* c, uint64_t seed, int32_t n_nodes, const int32_t* parent, const uint64_t* thr,
                             const uint8_t* emit, int64_t n_sites, uint8_t* packed, int64_t row_stride_bytes) {
  if (!c) return ABN_ERR_INVALID_ARG;
  const std::string why = sim_refusal(n_nodes, parent, thr, emit, n_sites, packed, row_stride_bytes);
  if (!why.empty()) return refused(c, why);
  if (n_sites == 0) return ABN_OK;
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    int64_t rows = 0;
    for (int32_t v = 0; v < n_nodes; ++v) rows += emit[v] != 0;
    const int64_t row_bytes = sim_row_bytes(n_sites);
    DevBuf<uint8_t> dout;
    HIPCHK(c, dout.alloc((size_t)rows * (size_t)row_bytes));
    if (int rc = sim_run(c, seed, n_nodes, parent, thr, emit, n_sites, dout.p, row_bytes, nullptr)) return rc;
    HIPCHK(c, hipMemcpy2DAsync(packed, (size_t)row_stride_bytes, dout.p, (size_t)row_bytes, (size_t)row_bytes, (size_t)rows,
                               hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ABN_OK;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_sim_pedigree(abn_ctx* c, uint64_t seed, int32_t n_nodes, const int32_t* parent, const int32_t* generation,
                                const uint64_t* thr, const uint8_t* emit, int64_t n_sites, double* rows, double* p0uu,
                                double* ms2) {
  if (!c) return ABN_ERR_INVALID_ARG;
  const std::string why = sim_refusal(n_nodes, parent, thr, emit, n_sites, nullptr, 0, false);
  if (!why.empty()) return refused(c, why);
  if (!generation || !rows || !p0uu) return refused(c, "abn_sim_pedigree: a null pointer");
  if (n_sites < 1) return refused(c, "abn_sim_pedigree: no site");
  std::vector<int32_t> sampled;
  for (int32_t v = 0; v < n_nodes; ++v)
    if (emit[v]) sampled.push_back(v);
  const int32_t n = (int32_t)sampled.size();
  if (n < 2) return refused(c, "abn_sim_pedigree: fewer than two emitted nodes");
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    const size_t pairs = (size_t)n * (size_t)(n - 1) / 2;
    const int64_t stride = sim_row_bytes(n_sites);
    DevBuf<uint8_t> dcodes;
    DevBuf<double> ddvalue;
    DevBuf<unsigned long long> dtable;
    double ms[2] = {0.0, 0.0};
    HIPCHK(c, dcodes.alloc((size_t)n * (size_t)stride));
    HIPCHK(c, ddvalue.alloc(pairs));
    HIPCHK(c, dtable.alloc(pairs * 9));
    if (int rc = sim_run(c, seed, n_nodes, parent, thr, emit, n_sites, dcodes.p, stride, &ms[0])) return rc;
    if (int rc = abn_pairwise_divergence_packed_dev(c, dcodes.p, n, n_sites, stride, nullptr, nullptr, ddvalue.p, &ms[1])) return rc;
    double table_ms = 0.0;  // the second pass over the matrix: the state counts behind p0uu
    if (int rc = transitions_packed_dev(c, dcodes.p, n, n_sites, stride, dtable.p, &table_ms)) return rc;
    ms[1] += table_ms;
    std::vector<double> dvalue(pairs);
    std::vector<unsigned long long> table(pairs * 9);
    if (int rc = to_host(c, dvalue.data(), ddvalue)) return rc;
    if (int rc = to_host(c, table.data(), dtable)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // DMatrix::convert's rows (src/pedigree.rs:281-333): the pairs i < j of the sampled nodes in their order
    size_t p = 0;
    for (int32_t i = 0; i < n; ++i)
      for (int32_t j = i + 1; j < n; ++j, ++p) {
        rows[4 * p + 0] = (double)sim_common_generation(parent, generation, sampled[(size_t)i], sampled[(size_t)j]);
        rows[4 * p + 1] = (double)generation[sampled[(size_t)i]];
        rows[4 * p + 2] = (double)generation[sampled[(size_t)j]];
        rows[4 * p + 3] = dvalue[p];
      }
    // rc_meth_lvl of a sample from the sums of the table of its pair with sample 0 (sample 0: with sample 1): a site's
    // level is state / 2, no site is filtered (src/pedigree.rs:171-183)
    double sum = 0.0;
    for (int32_t s = 0; s < n; ++s) {
      const unsigned long long* t = &table[9 * (size_t)(s == 0 ? 0 : s - 1)];  // pair (0, max(s, 1))
      unsigned long long n1 = 0, n2 = 0;
      for (int x = 0; x < 3; ++x) {
        n1 += s == 0 ? t[3 * 1 + x] : t[3 * x + 1];
        n2 += s == 0 ? t[3 * 2 + x] : t[3 * x + 2];
      }
      sum += 1.0 - (double)(n1 + 2 * n2) / (2.0 * (double)n_sites);
    }
    *p0uu = sum / (double)n;
    if (ms2) ms2[0] = ms[0], ms2[1] = ms[1];
    return ABN_OK;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_sim_obs_thresholds(const double miscall[9], const double dropout[3], uint64_t othr[9], char* text,
                                      int32_t text_bytes) {
  const std::string why = sim_obs_thresholds(miscall, dropout, othr);
  if (text && text_bytes > 0) snprintf(text, (size_t)text_bytes, "%s", why.c_str());
  return why.empty() ? ABN_OK : ABN_ERR_INVALID_ARG;
}

extern "C" int abn_sim_observe_dev(abn_ctx* c, uint64_t seed, int32_t n_rows, const int32_t* node_of_row, const uint64_t* othr,
                                   int64_t n_sites, const void* dev_in, int64_t in_stride, void* dev_out, int64_t out_stride,
                                   double* kernel_ms) {
  if (!c) return ABN_ERR_INVALID_ARG;
  const std::string why = sim_observe_refusal(n_rows, node_of_row, othr, n_sites, dev_in, in_stride, dev_out, out_stride);
  if (!why.empty()) return refused(c, why);
  if ((((uintptr_t)dev_in | (uintptr_t)dev_out) & 15u) != 0)
    return refused(c, "abn_sim_observe_dev: dev_in or dev_out is not 16-byte aligned");
  if (kernel_ms) *kernel_ms = 0.0;
  if (n_sites == 0) return ABN_OK;
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    return observe_run(c, seed, n_rows, node_of_row, othr, n_sites, (const uint8_t*)dev_in, in_stride, (uint8_t*)dev_out,
                       out_stride, kernel_ms);
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_sim_observe(abn_ctx* c, uint64_t seed, int32_t n_rows, const int32_t* node_of_row, const uint64_t* othr,
                               int64_t n_sites, const uint8_t* packed_in, int64_t in_stride, uint8_t* packed_out,
                               int64_t out_stride) {
  if (!c) return ABN_ERR_INVALID_ARG;
  const std::string why = sim_observe_refusal(n_rows, node_of_row, othr, n_sites, packed_in, in_stride, packed_out, out_stride);
  if (!why.empty()) return refused(c, why);
  if (n_sites == 0) return ABN_OK;
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    const int64_t row_bytes = sim_row_bytes(n_sites);
    DevBuf<uint8_t> d;  // observed in place on the device
    HIPCHK(c, d.alloc((size_t)n_rows * (size_t)row_bytes));
    HIPCHK(c, hipMemcpy2DAsync(d.p, (size_t)row_bytes, packed_in, (size_t)in_stride, (size_t)row_bytes, (size_t)n_rows,
                               hipMemcpyHostToDevice, c->stream));
    if (int rc = observe_run(c, seed, n_rows, node_of_row, othr, n_sites, d.p, row_bytes, d.p, row_bytes, nullptr)) return rc;
    HIPCHK(c, hipMemcpy2DAsync(packed_out, (size_t)out_stride, d.p, (size_t)row_bytes, (size_t)row_bytes, (size_t)n_rows,
                               hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ABN_OK;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}

extern "C" int abn_sim_study(abn_ctx* c, uint64_t seed, int32_t n_nodes, const int32_t* parent, const int32_t* generation,
                             const uint64_t* thr, const uint8_t* emit, const uint64_t* othr, int64_t n_sites, int32_t n_replicates,
                             double* times, double* dvalue, double* p0uu, uint64_t* census, double* ms4) {
  if (!c) return ABN_ERR_INVALID_ARG;
  const std::string why = sim_refusal(n_nodes, parent, thr, emit, 0, nullptr, 0, false);
  if (!why.empty()) return refused(c, why);
  if (!generation || !times || !dvalue || !p0uu) return refused(c, "abn_sim_study: a null pointer");
  if (n_sites < 1) return refused(c, "abn_sim_study: no site");
  if (n_replicates < 1) return refused(c, "abn_sim_study: fewer than one replicate");
  if (n_sites > kSimMaxSites / n_replicates)
    return refused(c, "abn_sim_study: n_replicates x n_sites lies above 2^34");
  std::vector<int32_t> sampled;
  for (int32_t v = 0; v < n_nodes; ++v)
    if (emit[v]) sampled.push_back(v);
  const int32_t n = (int32_t)sampled.size();
  if (n < 2) return refused(c, "abn_sim_study: fewer than two emitted nodes");
  if (othr)
    for (int s = 0; s < 3; ++s)
      if (othr[3 * s] > othr[3 * s + 1] || othr[3 * s + 1] > othr[3 * s + 2])
        return refused(c, "abn_sim_study: othr[" + std::to_string(s) + "] decreases");
  try {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    const int64_t R = n_replicates, total = R * n_sites, stride = sim_row_bytes(total);
    const size_t pairs = (size_t)n * (size_t)(n - 1) / 2;
    std::vector<int64_t> begin((size_t)R), end((size_t)R);
    for (int64_t r = 0; r < R; ++r) begin[(size_t)r] = r * n_sites, end[(size_t)r] = (r + 1) * n_sites;
    DevBuf<uint8_t> dcodes;
    DevBuf<double> ddvalue;
    DevBuf<unsigned long long> dcounts;
    double ms[4] = {0.0, 0.0, 0.0, 0.0};
    HIPCHK(c, dcodes.alloc((size_t)n * (size_t)stride));
    HIPCHK(c, ddvalue.alloc((size_t)R * pairs));
    HIPCHK(c, dcounts.alloc((size_t)R * (size_t)n * 3));
    if (int rc = sim_run(c, seed, n_nodes, parent, thr, emit, total, dcodes.p, stride, &ms[0])) return rc;
    if (othr)
      if (int rc = observe_run(c, seed, n, sampled.data(), othr, total, dcodes.p, stride, dcodes.p, stride, &ms[1])) return rc;
    if (int rc = pairwise_windows_packed_dev(c, dcodes.p, n, total, stride, begin.data(), end.data(), n_replicates, nullptr, nullptr,
                                             ddvalue.p, &ms[2]))
      return rc;
    if (int rc = packed_census_windows_dev(c, dcodes.p, n, total, stride, begin.data(), end.data(), n_replicates, dcounts.p, &ms[3]))
      return rc;
    std::vector<unsigned long long> counts((size_t)R * (size_t)n * 3);
    if (int rc = to_host(c, dvalue, ddvalue)) return rc;
    if (int rc = to_host(c, counts.data(), dcounts)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // DMatrix::convert's times (src/pedigree.rs:281-333): the pairs i < j of the sampled nodes in their order
    size_t p = 0;
    for (int32_t i = 0; i < n; ++i)
      for (int32_t j = i + 1; j < n; ++j, ++p) {
        times[3 * p + 0] = (double)sim_common_generation(parent, generation, sampled[(size_t)i], sampled[(size_t)j]);
        times[3 * p + 1] = (double)generation[sampled[(size_t)i]];
        times[3 * p + 2] = (double)generation[sampled[(size_t)j]];
      }
    // rc_meth_lvl of a sample over its own kept sites (src/pedigree.rs:159-175): a level is state / 2; a sample that keeps
    // nothing gives the reference's 0 / 0
    for (int64_t r = 0; r < R; ++r) {
      double sum = 0.0;
      for (int32_t s = 0; s < n; ++s) {
        const unsigned long long* k = &counts[((size_t)r * (size_t)n + (size_t)s) * 3];
        sum += 1.0 - (double)(k[1] + 2 * k[2]) / (2.0 * (double)(k[0] + k[1] + k[2]));
      }
      p0uu[r] = sum / (double)n;
    }
    if (census) std::copy(counts.begin(), counts.end(), census);
    if (ms4) std::copy(ms, ms + 4, ms4);
    return ABN_OK;
  } catch (const std::bad_alloc&) {
    return set_err(c, ABN_ERR_HIP, "out of host memory");
  }
}
