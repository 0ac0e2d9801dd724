// The fit path's kernels in libabneutral_hip.so: the one translation unit that includes abn_device.hpp — the table of every
// fit-kernel instantiation, the launchers around it (declared in abn_fit_host.hpp; abn_plan.hip launches through them), and
// the one-shot entries of the C-ABI (include/abneutral.h) that launch directly.  No CPU compute path exists here by design:
// if HIP is unusable every compute entry point returns ABN_ERR_NO_DEVICE / ABN_ERR_HIP.
#include <functional>

#include "abn_fit_host.hpp"
#include "abn_device.hpp"

using namespace abn;

static_assert(sizeof(abn_fit_info) == sizeof(FitInfoDev), "abn_fit_info layout");

// ------------------------------------------------------------------------------------------------
// launchers: abn_route.hpp decides, this executes
// ------------------------------------------------------------------------------------------------
static hipError_t allow_lds(const void* kernel, size_t lds) {
  if (lds <= kDefaultDynLds) return hipSuccess;
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// key -> kernel, written once: every fit-path instantiation the library holds (tests/test_kernel_matrix_census.py counts
// them in the assembly), those no route reaches included (tests/_kernel_matrix.py: UNREACHABLE)
struct KernelEntry {
  KernelKey key;
  const void* fn;
};
#define ABN_FIT(G, R, TP, ST) {{kFamFit, G, R, TP, ST, false}, reinterpret_cast<const void*>(&abn_fit_kernel<G, R, TP, ST>)}
#define ABN_FIT_ROWS(G, TP, ST) ABN_FIT(G, 1, TP, ST), ABN_FIT(G, 2, TP, ST), ABN_FIT(G, 4, TP, ST), ABN_FIT(G, 8, TP, ST), ABN_FIT(G, 0, TP, ST)
#define ABN_FIT_G(G)                                                                                                   \
  ABN_FIT_ROWS(G, false, false), ABN_FIT(G, -1, false, false), ABN_FIT_ROWS(G, true, false), ABN_FIT(G, -1, true, false), \
      ABN_FIT_ROWS(G, false, true)
#define ABN_REFILL(G, R) {{kFamRefill, G, R, false, false, false}, reinterpret_cast<const void*>(&abn_fit_refill_kernel<G, R>)}
#define ABN_REFILL_G(G) ABN_REFILL(G, 1), ABN_REFILL(G, 2), ABN_REFILL(G, 4), ABN_REFILL(G, 8)
#define ABN_SPEC(R, ST, RS) {{kFamSpec, kWave, R, false, ST, RS}, reinterpret_cast<const void*>(&abn_fit_spec_kernel<R, ST, RS>)}
#define ABN_SPEC_R(R) ABN_SPEC(R, false, false), ABN_SPEC(R, true, false), ABN_SPEC(R, false, true)
#define ABN_COST(G) {{kFamCost, G, 0, false, false, false}, reinterpret_cast<const void*>(&abn_cost_kernel<G>)}
#define ABN_SWEEP(R) {{kFamSweep, kWave, R, false, false, false}, reinterpret_cast<const void*>(&abn_sweep_kernel<R>)}
static const KernelEntry kKernels[] = {
    ABN_FIT_G(8), ABN_FIT_G(16), ABN_FIT_G(32), ABN_FIT_G(64),
    ABN_FIT(64, 16, false, false), ABN_FIT(64, 16, true, false), ABN_FIT(64, 16, false, true),  // one wavefront per chain only
    ABN_REFILL_G(8), ABN_REFILL_G(16), ABN_REFILL_G(32), ABN_REFILL_G(64),
    ABN_SPEC_R(1), ABN_SPEC_R(2), ABN_SPEC_R(4), ABN_SPEC_R(8),
    ABN_COST(8), ABN_COST(16), ABN_COST(32), ABN_COST(64),
    ABN_SWEEP(0), ABN_SWEEP(-1)};
static_assert(sizeof(kKernels) / sizeof(kKernels[0]) == 103 + 2,
              "the census of tests/test_kernel_matrix_census.py, and the two sweep kernels of tests/test_stream_sweep_cpu.py");

template <class Args>
static int launch_route(abn_ctx* c, const LaunchRoute& r, const Args& a, hipStream_t st) {
  const void* fn = nullptr;
  for (const KernelEntry& e : kKernels)
    if (e.key == r.key) fn = e.fn;
  if (!fn) return set_err(c, ABN_ERR_INVALID_ARG, "internal: no such kernel instantiation");
  HIPCHK(c, allow_lds(fn, r.lds));
  void* argv[] = {const_cast<Args*>(&a)};
  HIPCHK(c, hipLaunchKernel(fn, dim3(r.grid), dim3(r.block), argv, r.lds, st));
  return ABN_OK;
}

// Fills the ranges of `l` on stream st: in one launch of abn_step_prepare_kernel, or (one_launch = false) as one memset
// per range — the same list either way.  A range outside its buffer is refused, not written, and so is a list that
// could not hold all of its ranges.
int abn::clear_ranges(abn_ctx* c, const PrepList& l, const PrepBases& b, hipStream_t st, bool one_launch) {
  if (l.overflow) return set_err(c, ABN_ERR_INVALID_ARG, "internal: a step's clears do not fit their list");
  PrepArgs pa{};
  unsigned long long most = 0;
  for (int k = 0; k < l.n; ++k) {
    const PrepRange& r = l.r[k];
    if (!b.base[r.buffer] || r.offset % 4 || r.bytes % 4 || r.offset + r.bytes > b.bytes[r.buffer])
      return set_err(c, ABN_ERR_INVALID_ARG, "internal: a step's clear lies outside its buffer");
    char* at = static_cast<char*>(b.base[r.buffer]) + r.offset;
    if (!one_launch) {
      HIPCHK(c, hipMemsetAsync(at, r.fill, r.bytes, st));
      continue;
    }
    pa.r[pa.n].p = reinterpret_cast<unsigned*>(at);
    pa.r[pa.n].words = r.bytes / 4;
    pa.r[pa.n].fill = 0x01010101u * r.fill;
    most = std::max(most, pa.r[pa.n].words / 4);
    ++pa.n;
  }
  if (pa.n == 0) return ABN_OK;
  const unsigned blocks = (unsigned)std::min<unsigned long long>(1024, std::max<unsigned long long>(1, (most + 255) / 256));
  hipLaunchKernelGGL(abn_step_prepare_kernel, dim3(blocks), dim3(256), 0, st, pa);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

// The chains parked in a's list (a.susp_list, a.susp_count) resume in the speculative kernel and run to their end: one
// workgroup per slot of the list up to `cap` (those beyond *a.susp_count leave at once)
int abn::launch_tail_resume(abn_ctx* c, const PedigreeRoute& pr, FitArgs a, int cap, hipStream_t st) {
  const LaunchRoute t = route_tail_resume(pr, cap);
  if (t.status) return set_err(c, t.status, t.error);
  a.chain_stride = t.chain_stride;
  a.tree = t.tree;
  a.queue = nullptr;
  a.quantum = 0;
  a.spec_resume = 1;
  return launch_route(c, t, a, st);
}

// Runs a.W x a.C chains as route_launch decides.  `a` carries the buffers `offer` promises (queue; park_*, state,
// susp_list, slice_status); chain_stride, tree, quantum, tail and pass are the route's and are set here.
// kind (nullable): the ABN_KERNEL_* code of what was launched (PERSISTENT: a.slice_status then counts its fits)
// lc: required where the offer admits a persistent launch (status words and FIFO must be clear before it)
int abn::launch_fit(abn_ctx* c, const PedigreeRoute& pr, const PhaseRoute& ph, FitArgs a, const LaunchOffer& offer,
                    hipStream_t st, int* kind, LaunchClear* lc) {
  const long long chains = (long long)a.W * a.C;
  LaunchRoute r = route_launch(pr, ph, chains, c->cus, offer);
  if (kind) *kind = r.kind;
  if (r.status) return set_err(c, r.status, r.error);
  if (r.kind == ABN_KERNEL_NONE) return ABN_OK;
  const bool persistent = r.kind == ABN_KERNEL_PERSISTENT;
#ifdef ABN_MEASUREMENT_KNOBS  // scripts/prio_sweep.sh, tail_sweep.sh: wave priority by chain age, wavefronts, quantum and tail of the persistent launch
  if (persistent) {
    if (const char* e = getenv("ABN_PRIO")) sscanf(e, "%d,%d,%d,%d", &a.prio_mode, &a.prio_t[0], &a.prio_t[1], &a.prio_t[2]);
    if (const char* e = getenv("ABN_PERSIST_WAVES_SMALL_ENV")) {
      if (r.grid == persist_waves_small(c->cus)) r.grid = (unsigned)std::max(64, atoi(e));
      if (r.tail_cap > 0) r.tail_cap = tail_cap_for(pr, r.grid, c->cus);
    }
    if (const char* e = getenv("ABN_QUANTUM_ENV")) {
      if (r.quantum > 0) r.quantum = std::max(16, atoi(e));
    }
    // tests/test_gpu_parity.py::test_lost_fifo_entry_is_an_error_at_sync: the first parked chain of FIFO shard 0 is never
    // published — the launch must end (bounded spin), and every way of taking results must report ABN_ERR_HIP
    if (const char* e = getenv("ABN_DROP_FIFO_ENTRY")) a.drop_entry = atoi(e);
    if (const char* e = getenv("ABN_TAIL_CAP")) {
      if (r.tail_cap > 0) r.tail_cap = (int)std::min<long long>(chains, std::max(0, atoi(e)));
    }
  }
#endif
  a.chain_stride = r.chain_stride;
  a.tree = r.tree;
  a.iter_cap = offer.pass == 1 ? kPhaseACap : 0;
  a.resume = offer.pass == 2 ? 1 : 0;
  a.quantum = r.quantum;
  a.tail_cap = r.tail_cap;
  if (!persistent) a.queue = nullptr;
  if (r.kind != ABN_KERNEL_STREAM_SWEEP) a.passes = nullptr;
  if (a.tail_cap > 0) a.susp_count = reinterpret_cast<int*>(a.slice_status + kSliceTailFill);
  {  // zeroed status words; an empty FIFO of parked chains (entries -1, head = tail = 0): whatever the head left to do
    const bool status = persistent && a.slice_status, fifo = a.quantum > 0;
    if ((status || fifo) && !lc) return set_err(c, ABN_ERR_INVALID_ARG, "internal: a persistent launch without its clears");
    if (lc) {
      bool& status_clean = lc->clean->status[lc->slot];
      bool& fifo_clean = lc->clean->fifo[lc->region];
      const PrepList l = prep_launch(lc->slot, status && !status_clean, fifo && !fifo_clean, (unsigned)a.park_cap, lc->region);
      if (int rc = clear_ranges(c, l, lc->bases, st)) return rc;
      if (status) status_clean = false;   // used
      if (fifo) fifo_clean = false;
    }
  }
  if (int rc = launch_route(c, r, a, st)) return rc;
  if (a.tail_cap > 0) return launch_tail_resume(c, pr, a, a.tail_cap, st);  // the parked tail (possibly empty)
  return ABN_OK;
}

// one model per workgroup, then one workgroup per window over its S sums
int abn::launch_select(abn_ctx* c, const SelectArgs& s, size_t lds, hipStream_t st) {
  HIPCHK(c, allow_lds(reinterpret_cast<const void*>(&abn_select_lse_kernel), lds));
  HIPCHK(c, allow_lds(reinterpret_cast<const void*>(&abn_select_kernel), lds));
  hipLaunchKernelGGL(abn_select_lse_kernel, dim3((unsigned)((long long)s.W * s.S)), dim3(kWave), lds, st, s);
  hipLaunchKernelGGL(abn_select_kernel, dim3((unsigned)s.W), dim3(kWave), lds, st, s);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

int abn::launch_gen_idx(abn_ctx* c, uint32_t* idx, int n, int b, int w, uint64_t seed, uint32_t woff, uint32_t boff,
                        const uint32_t* wid) {
  const long long total = (long long)w * b * ((n + 3) / 4);
  if (total <= 0) return ABN_OK;
  const long long want = (total + 255) / 256;
  const unsigned blocks = (unsigned)std::min<long long>(want, 32LL * c->cus);
  hipLaunchKernelGGL(abn_gen_idx_kernel, dim3(blocks), dim3(256), 0, c->stream, idx, n, b, w, seed, woff, boff, wid);
  HIPCHK(c, hipGetLastError());
  return ABN_OK;
}

// ------------------------------------------------------------------------------------------------
// one-shot entries
// ------------------------------------------------------------------------------------------------
// What abn_cost_batch, abn_fit_batch and abn_select_best start with once their arguments are checked: the device, the
// pool scope of the call, the topology of a four-column pedigree (refused with the status text) and its upload.
// `check` (optional) runs between the two: what the caller refuses before anything is uploaded.
struct OneShot {
  PoolScope pool_scope;
  Topology t;
  DevTopology dt;
  explicit OneShot(abn_ctx* c) : pool_scope(c) {}
  int open(abn_ctx* c, const double* pedigree, int n_rows, const std::function<int()>& check = nullptr) {
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = build_topology(pedigree, n_rows, 4, t)) return set_err(c, rc, abn_status_string(rc));
    if (check)
      if (int rc = check()) return rc;
    return upload_topology(c, t, dt);
  }
};

extern "C" int abn_gen_boot_indices(abn_ctx* c, uint64_t seed, uint32_t window, uint32_t b0, int64_t nb, int32_t n_rows,
                                    uint32_t* idx) {
  if (!c || !idx || nb < 0 || n_rows <= 0 || nb > 0x7fffffff) return ABN_ERR_INVALID_ARG;
  if (nb == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<uint32_t> d;
  HIPCHK(c, d.alloc((size_t)nb * (size_t)n_rows));
  int rc = launch_gen_idx(c, d.p, n_rows, (int)nb, 1, seed, window, b0);
  if (rc || (rc = to_host(c, idx, d))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}

// ------------------------------------------------------------------------------------------------
// (1) cost batch
// ------------------------------------------------------------------------------------------------
extern "C" int abn_cost_batch(abn_ctx* c, const abn_options* opts, const double* pedigree, int32_t n_rows, double p_uu0,
                              double eqp, double eqp_weight, const double* candidates, int64_t m, const double* pred,
                              const double* resid, const uint32_t* idx, const uint32_t* cand_to_boot,
                              int64_t n_boot_rows, double* cost, double* dt1t2, double* p_uu_inf) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (!pedigree || n_rows <= 0 || !candidates || m < 0 || !cost) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (idx && (!pred || !resid || n_boot_rows <= 0)) return set_err(c, ABN_ERR_INVALID_ARG, "bootstrap inputs");
  if (m == 0) return ABN_OK;
  if (const char* oe = options_error(resolve(opts))) return set_err(c, ABN_ERR_INVALID_ARG, oe);
  const abn_options o = resolve_for(opts, n_rows);
  OneShot s(c);
  int rc = s.open(c, pedigree, n_rows, [&]() -> int {
    for (int64_t i = 0; idx && i < m; ++i)
      if ((cand_to_boot ? (int64_t)cand_to_boot[i] : i) >= n_boot_rows)
        return set_err(c, ABN_ERR_INVALID_ARG, "cand_to_boot out of range");
    return ABN_OK;
  });
  if (rc) return rc;
  const size_t N = (size_t)n_rows;
  const std::vector<double> dcol = column3(pedigree, n_rows);
  DevBuf<double> dD, dpred, dresid, dcand, dcost, ddt, dpuu;
  DevBuf<uint32_t> didx, dc2b;
  if ((rc = upload(c, dD, dcol.data(), N)) || (rc = upload(c, dcand, candidates, (size_t)m * 4))) return rc;
  HIPCHK(c, dcost.alloc((size_t)m));
  if (idx) {
    if ((rc = upload(c, dpred, pred, N)) || (rc = upload(c, dresid, resid, N)) ||
        (rc = upload(c, didx, idx, (size_t)n_boot_rows * N)))
      return rc;
    for (size_t q = 0; q < (size_t)n_boot_rows * N; ++q)
      if (idx[q] >= (uint32_t)N) return set_err(c, ABN_ERR_INVALID_ARG, "bootstrap index out of range");
    if (cand_to_boot && (rc = upload(c, dc2b, cand_to_boot, (size_t)m))) return rc;
  }
  if (dt1t2) HIPCHK(c, ddt.alloc((size_t)m * N));
  if (p_uu_inf) HIPCHK(c, dpuu.alloc((size_t)m));

  const PedigreeRoute pr = route_pedigree(n_rows, s.t.K, s.t.T, o.lanes_per_chain, o.strict_order);
  if (pr.cost_refusal) return set_err(c, ABN_ERR_INVALID_ARG, pr.cost_refusal);
  const int ng = kWave / pr.cost_lanes;
  CostArgs a{};
  fill_topology(a, s.t, s.dt);
  a.chain_stride = s.t.chain_stride;
  a.p_uu0 = p_uu0;
  a.eqp = eqp;
  a.eqp_w = eqp_weight;
  a.D = dD.p;
  a.pred = dpred.p;
  a.resid = dresid.p;
  a.idx = didx.p;
  a.cand_to_boot = dc2b.p;
  a.dmode = idx ? 1 : 0;
  a.cand = dcand.p;
  a.M = m;
  a.strict = pr.strict;
  a.tree = pr.cost_tree;
  a.cost = dcost.p;
  a.dt = ddt.p;
  a.puu = dpuu.p;
  const long long blocks = (m + ng - 1) / ng;
  if (blocks > 0x7fffffffLL) return set_err(c, ABN_ERR_INVALID_ARG, "too many candidates");
  LaunchRoute r{};
  r.key = {kFamCost, pr.cost_lanes, 0, false, false, false};
  r.grid = (unsigned)blocks;
  r.block = kWave;
  r.lds = pr.cost_lds;
  rc = launch_route(c, r, a, c->stream);
  if (rc || (rc = to_host(c, cost, dcost)) || (rc = to_host(c, dt1t2, ddt)) || (rc = to_host(c, p_uu_inf, dpuu))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}

// ------------------------------------------------------------------------------------------------
// Nelder-Mead fit batch (explicit start simplices)
// ------------------------------------------------------------------------------------------------
// sweep: abn_fit_batch_sweep — the launch must take abn_sweep_kernel, or the call is refused; passes: its counter (nullable)
static int fit_batch(abn_ctx* c, const abn_options* opts, const double* pedigree, int32_t n_rows, double p_uu0, double eqp,
                     double eqp_weight, const double* simplex0, int64_t f, const double* dobs_rows, int32_t max_iters,
                     double* best, abn_fit_info* info, bool sweep, int64_t* passes) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (passes) *passes = 0;
  if (!pedigree || n_rows <= 0 || !simplex0 || f < 0 || !best || max_iters < 0 || f > 0x7fffffff)
    return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (f == 0) return ABN_OK;
  if (const char* oe = options_error(resolve(opts))) return set_err(c, ABN_ERR_INVALID_ARG, oe);
  const abn_options o = resolve_for(opts, n_rows);
  if (max_iters > (1 << 28)) return set_err(c, ABN_ERR_INVALID_ARG, "max_iters must be in 0 .. 2^28");
  OneShot s(c);
  int rc = s.open(c, pedigree, n_rows);
  if (rc) return rc;
  const size_t N = (size_t)n_rows;
  DevBuf<double> dD, ds0, dbest, dscal;
  DevBuf<FitInfoDev> dinfo;
  const std::vector<double> dcol = dobs_rows ? std::vector<double>() : column3(pedigree, n_rows);
  const double scal[3] = {p_uu0, eqp, eqp_weight};
  if ((rc = upload(c, dD, dobs_rows ? dobs_rows : dcol.data(), dobs_rows ? (size_t)f * N : N)) ||
      (rc = upload(c, ds0, simplex0, (size_t)f * 20)) || (rc = upload(c, dscal, scal, 3)))
    return rc;
  HIPCHK(c, dbest.alloc((size_t)f * 4));
  HIPCHK(c, dinfo.alloc((size_t)f));
  HIPCHK(c, hipMemsetAsync(dinfo.p, 0, dinfo.bytes(), c->stream));

  const PedigreeRoute pr = route_pedigree(n_rows, s.t.K, s.t.T, o.lanes_per_chain, o.strict_order);
  FitArgs a{};  // wstride 0: the one set of scalars for every chain; dmode 0, smode 0: D and simplex0 as given
  fill_topology(a, s.t, s.dt);
  fill_options(a, o, pr);
  a.p_uu = dscal.p;
  a.eqp = dscal.p + 1;
  a.eqp_w = dscal.p + 2;
  a.D = dD.p;
  a.simplex0 = ds0.p;
  a.W = dobs_rows ? (int)f : 1;  // one "window" per fit when each has its own observed divergences
  a.C = dobs_rows ? 1 : (int)f;
  a.max_iters = max_iters;
  a.best = dbest.p;
  a.info = dinfo.p;
  LaunchOffer offer;
  DevBuf<unsigned long long> dpasses;
  unsigned long long hpasses = 0;
  if (sweep) {
    offer.sweep = true;
    const LaunchRoute r = route_launch(pr, PhaseRoute{false, pr.lanes, false}, f, c->cus, offer);
    if (r.status) return set_err(c, r.status, r.error);
    if (r.kind != ABN_KERNEL_STREAM_SWEEP)
      return set_err(c, ABN_ERR_INVALID_ARG,
                     "abn_fit_batch_sweep: this pedigree and these options do not route to the sweep kernel (it takes streamed "
                     "pedigrees at 64 lanes per chain in tree order, within the LDS of a CU)");
    HIPCHK(c, dpasses.alloc(1));
    HIPCHK(c, hipMemsetAsync(dpasses.p, 0, dpasses.bytes(), c->stream));
    a.passes = dpasses.p;
  }
  rc = launch_fit(c, pr, PhaseRoute{false, pr.lanes, false}, a, offer, c->stream);
  if (rc || (rc = to_host(c, best, dbest)) || (rc = to_host(c, info, dinfo)) || (sweep && (rc = to_host(c, &hpasses, dpasses))))
    return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (passes) *passes = (int64_t)hpasses;
  return ABN_OK;
}

extern "C" int abn_fit_batch(abn_ctx* c, const abn_options* opts, const double* pedigree, int32_t n_rows, double p_uu0,
                             double eqp, double eqp_weight, const double* simplex0, int64_t f, const double* dobs_rows,
                             int32_t max_iters, double* best, abn_fit_info* info) {
  return fit_batch(c, opts, pedigree, n_rows, p_uu0, eqp, eqp_weight, simplex0, f, dobs_rows, max_iters, best, info, false, nullptr);
}

extern "C" int abn_fit_batch_sweep(abn_ctx* c, const abn_options* opts, const double* pedigree, int32_t n_rows, double p_uu0,
                                   double eqp, double eqp_weight, const double* simplex0, int64_t f, const double* dobs_rows,
                                   int32_t max_iters, double* best, abn_fit_info* info, int64_t* passes) {
  return fit_batch(c, opts, pedigree, n_rows, p_uu0, eqp, eqp_weight, simplex0, f, dobs_rows, max_iters, best, info, true, passes);
}

// ------------------------------------------------------------------------------------------------
// stand-alone selection and bootstrap rows
// ------------------------------------------------------------------------------------------------
extern "C" int abn_select_best(abn_ctx* c, const double* pedigree, int32_t n_rows, double p0uu, const double* models,
                               int32_t n_models, int32_t* best_index, double* model, double* pred, double* resid,
                               double* lse) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (!pedigree || n_rows <= 0 || !models || n_models <= 0 || !best_index)
    return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  OneShot s(c);
  PedigreeRoute pr{};
  int rc = s.open(c, pedigree, n_rows, [&]() -> int {
    pr = route_pedigree(n_rows, s.t.K, s.t.T, 0, 0);
    return pr.select_refusal ? set_err(c, ABN_ERR_INVALID_ARG, pr.select_refusal) : ABN_OK;
  });
  if (rc) return rc;
  const size_t N = (size_t)n_rows, S = (size_t)n_models;
  const std::vector<double> dcol = column3(pedigree, n_rows);
  DevBuf<double> dD, dm, dlse, dmodel, dpred, dresid, dp;
  DevBuf<FitInfoDev> dinfo;
  DevBuf<int32_t> dbest;
  if ((rc = upload(c, dD, dcol.data(), N)) || (rc = upload(c, dm, models, S * 4)) || (rc = upload(c, dp, &p0uu, 1)))
    return rc;
  HIPCHK(c, dlse.alloc(S));
  HIPCHK(c, dmodel.alloc(4));
  HIPCHK(c, dpred.alloc(N));
  HIPCHK(c, dresid.alloc(N));
  HIPCHK(c, dinfo.alloc(S));
  HIPCHK(c, dbest.alloc(1));
  HIPCHK(c, hipMemsetAsync(dinfo.p, 0, dinfo.bytes(), c->stream));  // status 0: every model is a candidate
  SelectArgs a{};
  fill_topology(a, s.t, s.dt);
  a.p_uu = dp.p;
  a.D = dD.p;
  a.models = dm.p;
  a.info = dinfo.p;
  a.W = 1;
  a.S = n_models;
  a.lse = dlse.p;
  a.model = dmodel.p;
  a.pred = dpred.p;
  a.resid = dresid.p;
  a.best_start = dbest.p;
  rc = launch_select(c, a, pr.select_lds, c->stream);
  if (rc || (rc = to_host(c, best_index, dbest)) || (rc = to_host(c, model, dmodel)) || (rc = to_host(c, pred, dpred)) ||
      (rc = to_host(c, resid, dresid)) || (rc = to_host(c, lse, dlse)))
    return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (*best_index < 0) return set_err(c, ABN_ERR_NO_FINITE_FIT, abn_status_string(ABN_ERR_NO_FINITE_FIT));
  return ABN_OK;
}

extern "C" int abn_bootstrap_rows(abn_ctx* c, const double* best, int64_t n_boot, double* raw) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (!best || !raw || n_boot < 0) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (n_boot == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<double> db, dr;
  if (int rc = upload(c, db, best, (size_t)n_boot * 4)) return rc;
  HIPCHK(c, dr.alloc((size_t)n_boot * 7));
  const unsigned blocks = (unsigned)std::min<long long>((n_boot + 255) / 256, 4096);
  hipLaunchKernelGGL(abn_rows_kernel, dim3(blocks), dim3(256), 0, c->stream, db.p, (long long)n_boot, dr.p);
  HIPCHK(c, hipGetLastError());
  if (int rc = to_host(c, raw, dr)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}
