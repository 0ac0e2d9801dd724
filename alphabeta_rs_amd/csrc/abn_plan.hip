// The device-resident plan of the C-ABI (include/abneutral.h: abn_plan_*) — its words, records and steps, the
// early-bootstraps run, what a caller takes results through — and the drop-in entries built on it (abn_ab_neutral_run,
// abn_boot_model_run).  Host code around the launchers of abn_api.hip (abn_fit_host.hpp); the three kernels only the plan
// launches are abn_plan_kernels.hpp's.
#include "abn_fit_host.hpp"
#include "abn_plan_kernels.hpp"

using namespace abn;

// ------------------------------------------------------------------------------------------------
// (4) device-resident plan
// ------------------------------------------------------------------------------------------------
// The plan's timing events: the fit launches of phase A, the selection, the fit launches of phase B.  One record where two
// spans meet: kEvSelect ends phase A's fits and starts the selection, and where phase B is enqueued right behind the
// selection (abn_plan_run) kEvFitB ends the selection too.  The phases run on their own (abn_plan_run_phase) do not meet:
// phase A then records kEvSelectEnd and phase B kEvFitBOwn, so that neither moves the other's span; the spans of
// PhaseRecord and abn_plan::select_span say which records bound the last run of each.
enum PlanEvent { kEvFitA, kEvSelect, kEvSelectEnd, kEvFitB, kEvFitBOwn, kEvFitBEnd, kPlanEvents };
struct EventSpan {
  int begin, end;  // PlanEvent
};

// What the last run of a phase (0 = A, 1 = B) did.  prepare_step opens it, launch_phase writes what was launched, end_step
// closes it; the sync (verify_persistent) adds what the device counted.  Nothing else writes it.
struct PhaseRecord {
  EventSpan span;               // the records around its fit launches
  bool ran = false;
  int32_t kind = 0, lanes = 0;  // ABN_KERNEL_* and lanes per chain of its last timed launch (abn_plan_last_kernels)
  long long expected = 0;       // chains its persistent launch had to finish (0: none was persistent)
  long long handed = 0;         // ... of which its tail handed to the speculative kernel (read at the last sync)
  bool sweep = false;           // a launch of it took abn_sweep_kernel
};
// Early bootstraps: whether the last run of phase B was an early run (the miss word then selects the slot of phase B),
// its starts parked at the quorum and its miss word (read at the last sync)
struct EarlyRecord {
  bool ran = false;
  int32_t parked = 0, miss = 0;
};

struct abn_plan {
  abn_ctx* ctx = nullptr;
  abn_options opt{};
  Topology topo;
  DevTopology dtopo;
  int N = 0, W = 0, S = 0, B = 0;
  uint32_t window_offset = 0, boot_offset = 0;
  PedigreeRoute route{};  // lanes, tree and what the pedigree admits (abn_route.hpp)
  std::vector<uint32_t> wid_host;  // Philox window ids (abn_plan_set_window_ids); empty = window_offset + w
  DevBuf<uint32_t> wid;
  bool windows_set = false;
  bool model_ready = false;  // a model is in place for phase B: phase A ran, or the caller uploaded one (plan_upload_model)
  DevBuf<double> D, pred, resid, p_uu, eqp, eqp_w, simplexA, bestA, model, lse, bestB, raw_own;
  DevBuf<FitInfoDev> infoA, infoB;
  DevBuf<int32_t> best_start;
  DevBuf<uint32_t> idx;
  DevBuf<double> dstar;  // stream mode: materialised bootstrap observations [W x B x N]
  DevBuf<double> nm_state;    // two-pass phase A: parked Nelder-Mead states [W x S x kStateDoubles]
  DevBuf<int> susp_list;      // [W x S] + 1 counter at the end
  // per phase (A, B) kPhaseWords words: kPhaseSkipped evaluations not executed (fixed-point skip), kPhaseQueue the chain
  // queue of the persistent kernel
  // ... one such slot per phase and one for the guarded redo of phase B (kPhaseSlots), then the words of the early
  // bootstraps (kEarlyWords) and the slots' status words (kSliceWords each): plan_words() lays the buffer out
  DevBuf<unsigned long long> skipped;
  bool twopass_a = false;
  DevBuf<int> slice_buf;      // time slicing: head, tail, then the FIFO of parked chains
  unsigned slice_cap = 0;
  bool stream_b = false;
  double* raw = nullptr;  // raw_own.p or caller-bound
  hipEvent_t ev[kPlanEvents] = {};
  PhaseRecord rec[2] = {{{kEvFitA, kEvSelect}}, {{kEvFitB, kEvFitBEnd}}};
  EventSpan select_span{kEvSelect, kEvSelectEnd};  // the records around the last selection
  EarlyRecord early_rec;
  // What the head of the running step has cleared (prep_clean of its list) and no launch has used since: launch_phase
  // hands it to launch_fit, which clears what is not
  PrepClean clean;
  hipEvent_t ev_fork = nullptr;
  std::vector<hipEvent_t> ev_join;
  // Early bootstraps (abn_plan_run; route_early_bootstraps): phase B launched on a quorum of the starts
  EarlyRoute early{};
  int early_mode = 1;                 // abn_plan_set_early_bootstraps: 0 off, 1 auto
  DevBuf<double> early_state;         // [S x kStateDoubles] the starts parked at the quorum (phase B parks in nm_state)
  DevBuf<int> early_list;             // [S] their list
  DevBuf<double> sel_model, sel_pred, sel_resid;   // the selection over all starts, made beside the early phase B
  DevBuf<int32_t> sel_best;
  // Stream sweep (abn_plan_set_stream_sweep): the mode and the device counter of each phase's passes over the rows
  // (allocated when the mode is first switched on)
  int sweep_mode = 0;
  DevBuf<unsigned long long> sweep_passes;
};

// The plan's small words (abn_prepare.hpp: kPlanWords64, and what a step clears of them)
static unsigned* early_words(const abn_plan* p) { return reinterpret_cast<unsigned*>(p->skipped.p + kPhaseSlots * kPhaseWords); }
static unsigned* slice_words(const abn_plan* p, int slot) { return early_words(p) + kEarlyWords + kSliceWords * slot; }
// what fetch_words copies: the whole of it
struct PlanWordsHost {
  unsigned long long phase[kPhaseSlots][kPhaseWords];
  unsigned early[kEarlyWords];
  unsigned slice[kPhaseSlots][kSliceWords];
};
static_assert(offsetof(PlanWordsHost, early) == kPlanEarlyOffset && offsetof(PlanWordsHost, slice) == plan_status_offset(0) &&
                  offsetof(PlanWordsHost, slice[kSlotRedo]) == plan_status_offset(kSlotRedo),
              "abn_prepare.hpp addresses the same words");
static_assert(sizeof(PlanWordsHost) <= kPlanWords64 * sizeof(unsigned long long) && sizeof(PlanWordsHost) % 8 == 0 &&
                  offsetof(PlanWordsHost, early) == kPhaseSlots * kPhaseWords * sizeof(unsigned long long) &&
                  offsetof(PlanWordsHost, slice) == offsetof(PlanWordsHost, early) + kEarlyWords * sizeof(unsigned),
              "PlanWordsHost mirrors the plan's words");
// enqueues the copy of the plan's words on the context's stream: h holds them once the caller has synchronised it
static int fetch_words(const abn_plan* p, PlanWordsHost& h) { return to_host(p->ctx, &h, p->skipped.p, sizeof h); }
// The slot whose words are those of the last run of `phase`: the phase's own, but the redo's for a phase B whose early
// run missed — that launch was stopped, and the redo's words are those of one complete phase B
static int phase_slot(const abn_plan* p, int phase, const PlanWordsHost& h) {
  return phase == 1 && p->early_rec.ran && h.early[kEarlyMiss] != 0 ? kSlotRedo : phase;
}

extern "C" int abn_plan_destroy(abn_plan* p) {
  if (!p) return ABN_ERR_INVALID_ARG;
  for (auto& e : p->ev)
    if (e) (void)hipEventDestroy(e);
  if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
  for (auto e : p->ev_join) (void)hipEventDestroy(e);
  delete p;
  return ABN_OK;
}

extern "C" int abn_plan_create(abn_ctx* c, const abn_options* opts, const double* generations, int32_t n_rows,
                               int32_t n_windows, int32_t n_starts, int32_t n_boot, uint32_t window_offset,
                               uint32_t boot_offset, abn_plan** out) {
  if (!c || !out) return ABN_ERR_INVALID_ARG;
  *out = nullptr;
  if (!generations || n_rows <= 0 || n_windows <= 0 || n_starts < 0 || n_boot < 0)
    return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if ((long long)n_windows * std::max(n_starts, n_boot) > 0x7fffffffLL)
    return set_err(c, ABN_ERR_INVALID_ARG, "too many chains");
  {
    const abn_options o = resolve(opts);
    if (const char* oe = options_error(o)) return set_err(c, ABN_ERR_INVALID_ARG, oe);
  }
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  struct Destroy {
    void operator()(abn_plan* q) const { abn_plan_destroy(q); }
  };
  std::unique_ptr<abn_plan, Destroy> owner(new (std::nothrow) abn_plan());  // every early return below destroys the plan
  abn_plan* p = owner.get();
  if (!p) return ABN_ERR_HIP;
  p->ctx = c;
  p->opt = resolve_for(opts, n_rows);  // strict_order resolved to 0 / 1 for this pedigree
  p->N = n_rows;
  p->W = n_windows;
  p->S = n_starts;
  p->B = n_boot;
  p->window_offset = window_offset;
  p->boot_offset = boot_offset;
  int rc = build_topology(generations, n_rows, 3, p->topo);
  if (rc) return set_err(c, rc, abn_status_string(rc));
  // what runs is a function of the pedigree and the options, decided (and refused) here, not at the first run
  p->route = route_pedigree(n_rows, p->topo.K, p->topo.T, p->opt.lanes_per_chain, p->opt.strict_order);
  if (p->route.refusal) return set_err(c, ABN_ERR_INVALID_ARG, p->route.refusal);
  auto fail = [&](hipError_t e, const char* what) {
    return set_err(c, ABN_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  };
  rc = upload_topology(c, p->topo, p->dtopo);
  if (rc) return rc;
  const size_t W = (size_t)n_windows, N = (size_t)n_rows, S = (size_t)n_starts, B = (size_t)n_boot;
  hipError_t e;
#define PALLOC(buf, count)                         \
  if ((e = p->buf.alloc(count)) != hipSuccess) return fail(e, "hipMalloc " #buf)
  PALLOC(D, W * N);
  PALLOC(pred, W * N);
  PALLOC(resid, W * N);
  PALLOC(p_uu, W);
  PALLOC(eqp, W);
  PALLOC(eqp_w, W);
  PALLOC(model, W * 4);
  PALLOC(best_start, W);
  PALLOC(simplexA, W * S * 20);
  PALLOC(bestA, W * S * 4);
  PALLOC(infoA, W * S);
  PALLOC(lse, W * S);
  PALLOC(idx, W * B * N);
  PALLOC(bestB, W * B * 4);
  PALLOC(infoB, W * B);
  PALLOC(raw_own, W * B * 7);
  PALLOC(skipped, kPlanWords64);
  p->twopass_a = plan_two_pass((long long)n_windows * n_starts, p->opt.max_iters_start, p->opt.no_fixed_point_skip,
                               p->opt.shrink_on_failed_contraction, p->opt.strict_order);
  if (p->twopass_a) {
    PALLOC(nm_state, W * S * kStateDoubles);
    PALLOC(susp_list, W * S + 1);
  }
  // time slicing for launches that outgrow the resident set of the persistent kernel: parked states, the FIFOs, the tail list
  if (const size_t chains = plan_sliced_chains(p->route, W * std::max(S, B), c->cus, p->opt.window_groups)) {
    if (p->nm_state.n < chains * kStateDoubles) PALLOC(nm_state, chains * kStateDoubles);
    p->slice_cap = (unsigned)(chains * 16 / kParkShards + 4096);   // per shard; a full shard just stops parking
    if (p->susp_list.n < chains + 1) PALLOC(susp_list, chains + 1);  // the tail list of the hand-over to the speculative kernel
  }
  p->stream_b = n_boot > 0 && p->route.streams && p->opt.stream_mode == 0;
  if (p->stream_b) PALLOC(dstar, W * B * N);
  p->early = route_early_bootstraps(p->route, n_windows, n_starts, n_boot, c->cus, p->opt.window_groups, p->twopass_a,
                                    p->slice_cap > 0);
  // route_early_bootstraps routed phase B on its resident observations (dmode 1).  A plan that materialises them (dmode 2)
  // streams its pedigree and so never runs persistent — and a phase B that is not persistent has no guard and would run
  // twice: held here, not left to follow from the route.
  if (p->stream_b) p->early = EarlyRoute{false, 0};
#ifdef ABN_MEASUREMENT_KNOBS  // a forced kernel is not what route_early_bootstraps assumed
  if (getenv("ABN_PHASE_A_KERNEL") || getenv("ABN_PHASE_B_KERNEL")) p->early = EarlyRoute{false, 0};
#endif
  // the FIFO: one region, and for an eligible plan a second one of the same size for the guarded redo (abn_prepare.hpp)
  if (p->slice_cap > 0) PALLOC(slice_buf, fifo_bytes(p->slice_cap, p->early.eligible) / sizeof(int));
  if (p->early.eligible) {
    PALLOC(early_state, S * kStateDoubles);
    PALLOC(early_list, S);
    PALLOC(sel_model, W * 4);
    PALLOC(sel_pred, W * N);
    PALLOC(sel_resid, W * N);
    PALLOC(sel_best, W);
  }
#undef PALLOC
  p->raw = p->raw_own.p;
  for (auto& ev : p->ev)
    if ((e = hipEventCreate(&ev)) != hipSuccess) return fail(e, "hipEventCreate");
  *out = owner.release();
  return ABN_OK;
}

// What plan_upload_model and abn_plan_set_windows end with, behind their own uploads: the per-window scalars, the
// bootstrap indices, and the stream synchronised (the callers' host temporaries may go).  The windows are then set;
// whether a model is ready is the caller's to say.
static int plan_set_scalars(abn_plan* p, const double* p0uu, const double* eqp, const double* eqp_w) {
  abn_ctx* c = p->ctx;
  const size_t W = (size_t)p->W;
  HIPCHK(c, hipMemcpyAsync(p->p_uu.p, p0uu, W * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(p->eqp.p, eqp, W * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(p->eqp_w.p, eqp_w, W * sizeof(double), hipMemcpyHostToDevice, c->stream));
  int rc = launch_gen_idx(c, p->idx.p, p->N, p->B, p->W, p->opt.seed, p->window_offset, p->boot_offset, p->wid.p);
  if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  p->windows_set = true;
  return ABN_OK;
}

static int plan_upload_model(abn_plan* p, const double* model, const double* pred, const double* resid,
                             const double* p0uu, const double* eqp, const double* eqp_w) {
  abn_ctx* c = p->ctx;
  HIPCHK(c, hipMemcpyAsync(p->model.p, model, p->model.bytes(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(p->pred.p, pred, p->pred.bytes(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(p->resid.p, resid, p->resid.bytes(), hipMemcpyHostToDevice, c->stream));
  if (int rc = plan_set_scalars(p, p0uu, eqp, eqp_w)) return rc;
  p->model_ready = true;
  return ABN_OK;
}

extern "C" int abn_plan_set_window_ids(abn_plan* p, const uint32_t* ids) {
  if (!p) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = p->ctx;
  if (p->windows_set) return set_err(c, ABN_ERR_STATE, "abn_plan_set_window_ids must precede abn_plan_set_windows");
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  if (!ids) {
    p->wid_host.clear();
    p->wid.release();
    return ABN_OK;
  }
  p->wid_host.assign(ids, ids + p->W);
  if (int rc = upload(c, p->wid, p->wid_host.data(), (size_t)p->W)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}

extern "C" int abn_plan_set_windows(abn_plan* p, const double* d_obs, const double* p0uu, const double* eqp,
                                    const double* eqp_weight) {
  if (!p) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = p->ctx;
  if (!d_obs || !p0uu) return set_err(c, ABN_ERR_INVALID_ARG, "null window data");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t W = (size_t)p->W, N = (size_t)p->N, S = (size_t)p->S;
  std::vector<double> ones(W, 1.0);  // eqp_weight = 1.0, src/alphabeta.rs:37,50
  const double* e1 = eqp ? eqp : p0uu;  // eqp = p0uu, src/alphabeta.rs:36,49
  const double* e2 = eqp_weight ? eqp_weight : ones.data();
  HIPCHK(c, hipMemcpyAsync(p->D.p, d_obs, p->D.bytes(), hipMemcpyHostToDevice, c->stream));
  std::vector<double> sx(W * S * 20);
  for (size_t w = 0; w < W; ++w) {
    double mx = d_obs[w * N];  // max of column 3, src/ab_neutral.rs:25-29
    for (size_t i = 1; i < N; ++i) mx = std::max(mx, d_obs[w * N + i]);
    const uint32_t wg = p->wid_host.empty() ? p->window_offset + (uint32_t)w : p->wid_host[w];
    abn_gen_start_simplices(p->opt.seed, wg, p->S, mx, sx.data() + w * S * 20);
  }
  if (!sx.empty())
    HIPCHK(c, hipMemcpyAsync(p->simplexA.p, sx.data(), p->simplexA.bytes(), hipMemcpyHostToDevice, c->stream));
  if (int rc = plan_set_scalars(p, p0uu, e1, e2)) return rc;  // synchronises: sx / ones are host temporaries
  p->model_ready = false;
  return ABN_OK;
}

// element offsets of window w0 in the plan's buffers: per window, per pedigree row, per start and per bootstrap
struct WindowOffsets {
  size_t w, rows, starts, boots;
};
static WindowOffsets window_offsets(const abn_plan* p, int w0) {
  const size_t o = (size_t)w0;
  return {o, o * (size_t)p->N, o * (size_t)p->S, o * (size_t)p->B};
}

// The FitArgs of windows [w0, w0 + wn) for phase 0 = A (starts) or 1 = B (bootstraps): every slice of the plan's buffers
// is taken here.  What a launch decides (chain_stride, tree, quantum, ...) is launch_fit's, what it is offered launch_phase's.
static FitArgs phase_args(const abn_plan* p, int phase, int w0, int wn) {
  const WindowOffsets o = window_offsets(p, w0);
  const size_t chains = phase ? o.boots : o.starts;
  FitArgs a{};
  fill_topology(a, p->topo, p->dtopo);
  fill_options(a, p->opt, p->route);
  a.p_uu = p->p_uu.p + o.w;
  a.eqp = p->eqp.p + o.w;
  a.eqp_w = p->eqp_w.p + o.w;
  a.wstride = 1;
  a.D = p->D.p + o.rows;
  a.pred = p->pred.p + o.rows;
  a.resid = p->resid.p + o.rows;
  a.idx = p->idx.p + o.boots * (size_t)p->N;
  a.model = p->model.p + o.w * 4;
  a.window_offset = p->window_offset + (uint32_t)w0;
  a.boot_offset = p->boot_offset;
  a.wid = p->wid.p ? p->wid.p + o.w : nullptr;
  a.W = wn;
  a.C = phase ? p->B : p->S;
  a.dmode = a.smode = phase;  // A: D and the start simplices as given; B: pred + resampled resid, simplices from Philox
  a.simplex0 = phase ? nullptr : p->simplexA.p + chains * 20;
  a.max_iters = phase ? p->opt.max_iters_boot : p->opt.max_iters_start;
  a.best = (phase ? p->bestB.p : p->bestA.p) + chains * 4;
  a.info = (phase ? p->infoB.p : p->infoA.p) + chains;
  a.raw = phase ? p->raw + chains * 7 : nullptr;
  return a;
}

static PrepBases prep_bases(const abn_plan* p) {
  PrepBases b;
  b.base[kPrepWords] = p->skipped.p;
  b.bytes[kPrepWords] = p->skipped.bytes();
  b.base[kPrepFifo] = p->slice_buf.p;
  b.bytes[kPrepFifo] = p->slice_buf.bytes();
  b.base[kPrepSweep] = p->sweep_passes.p;
  b.bytes[kPrepSweep] = p->sweep_passes.bytes();
  b.base[kPrepTail] = p->susp_list.p;
  b.bytes[kPrepTail] = p->susp_list.bytes();
  return b;
}

// The fit launch(es) of one phase (0 = A, 1 = B) for the windows `a` covers, on stream st.  A launch that covers the whole
// plan is offered the phase's chain queue, the plan's parking buffers and its status words; window groups on side streams
// would share them, so they get none (no persistent kernel, nothing to verify).
// slot: which of the plan's kPhaseSlots sets of words the launch counts in (the phase itself; kSlotRedo: the guarded redo)
// Writes the launch's part of the phase's record (PhaseRecord); timed: this launch is the one abn_plan_last_kernels names.
static int launch_phase(abn_plan* p, int phase, FitArgs& a, hipStream_t st, bool timed, int slot = -1) {
  abn_ctx* c = p->ctx;
  if (slot < 0) slot = phase;
  const bool whole = a.W == p->W;
  const char* force = nullptr;
#ifdef ABN_MEASUREMENT_KNOBS  // ABN_PHASE_A_KERNEL / ABN_PHASE_B_KERNEL = spec | wide | packed  (scripts/phase_a_sweep.py)
  force = getenv(phase ? "ABN_PHASE_B_KERNEL" : "ABN_PHASE_A_KERNEL");
#endif
  const PhaseRoute ph = route_phase(p->route, phase, (long long)p->W * (phase ? p->B : p->S), c->cus, a.dmode, whole,
                                    p->twopass_a, force);
  LaunchOffer offer;
  offer.queue = whole;
  offer.parking = whole && p->slice_cap > 0;
  offer.sweep = p->sweep_mode != 0;
  a.passes = p->sweep_passes.p ? p->sweep_passes.p + phase : nullptr;
  a.skipped = p->skipped.p + kPhaseWords * slot + kPhaseSkipped;
  if (whole) {
    a.queue = reinterpret_cast<unsigned*>(p->skipped.p + kPhaseWords * slot + kPhaseQueue);
    a.slice_status = slice_words(p, slot);
  }
  // only a launch of the whole plan may be persistent and use the plan's status words and FIFO
  const int region = fifo_region_of(slot, p->early.eligible);
  LaunchClear plan_lc{prep_bases(p), &p->clean, slot, region};
  LaunchClear* lc = whole ? &plan_lc : nullptr;
  if (offer.parking) {
    a.park_cap = p->slice_cap;
    a.park_ht = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(p->slice_buf.p) + fifo_header_offset(p->slice_cap, region));
    a.parked = reinterpret_cast<int*>(reinterpret_cast<char*>(p->slice_buf.p) + fifo_entries_offset(p->slice_cap, region));
    a.state = p->nm_state.p;
    a.susp_list = p->susp_list.p;   // tail hand-over (the route decides whether it applies)
  }
  if (a.quorum_words) {   // early bootstraps: the starts parked at the quorum have buffers of their own (phase B parks meanwhile)
    a.state = p->early_state.p;
    a.susp_list = p->early_list.p;
    a.susp_count = reinterpret_cast<int*>(early_words(p) + kEarlyParked);
  }
  int kind = ABN_KERNEL_NONE, rc;
  if (ph.two_pass) {
    int* cnt = p->susp_list.p + (size_t)p->W * (size_t)p->S;
    if (!p->clean.two_pass) {
      PrepList l;
      prep_two_pass(l, (size_t)p->W * (size_t)p->S);
      if ((rc = clear_ranges(c, l, plan_lc.bases, st))) return rc;
    }
    p->clean.two_pass = false;   // used
    a.state = p->nm_state.p;
    a.susp_list = p->susp_list.p;
    a.susp_count = cnt;
    offer.pass = 1;
    rc = launch_fit(c, p->route, ph, a, offer, st, &kind, lc);   // everybody, capped
    offer.pass = 2;
    if (!rc) rc = launch_fit(c, p->route, ph, a, offer, st, nullptr, lc);  // the parked chains, to the end
  } else {
    rc = launch_fit(c, p->route, ph, a, offer, st, &kind, lc);
  }
  if (rc) return rc;
  PhaseRecord& rec = p->rec[phase];
  if (whole) rec.expected = kind == ABN_KERNEL_PERSISTENT ? (long long)a.W * a.C : 0;
  if (kind == ABN_KERNEL_STREAM_SWEEP) rec.sweep = true;
  if (timed) {
    rec.kind = kind;
    rec.lanes = ph.lanes;
  }
  return ABN_OK;
}

// the selection of windows [w0, w0 + wn) over the fitted starts, into the plan's buffers
static SelectArgs select_args(const abn_plan* p, int w0, int wn) {
  const WindowOffsets o = window_offsets(p, w0);
  SelectArgs s{};
  fill_topology(s, p->topo, p->dtopo);
  s.p_uu = p->p_uu.p + o.w;
  s.D = p->D.p + o.rows;
  s.models = p->bestA.p + o.starts * 4;
  s.info = p->infoA.p + o.starts;
  s.W = wn;
  s.S = p->S;
  s.lse = p->lse.p + o.starts;
  s.model = p->model.p + o.w * 4;
  s.pred = p->pred.p + o.rows;
  s.resid = p->resid.p + o.rows;
  s.best_start = p->best_start.p + o.w;
  return s;
}

// Phase A (starts) + selection for windows [w0, w0+wn) on stream st.  timed: record the plan's timing events around
// the kernels.  early (abn_plan_run with early bootstraps, one window): the fit launch ends once the plan's quorum of
// starts has finished — the others park —, and the selection is over the finished ones.
// b_follows: phase B is enqueued on st right behind the selection, and its first record closes the selection's span too.
static int enqueue_phase_a(abn_plan* p, int w0, int wn, hipStream_t st, bool timed, bool b_follows, bool early = false) {
  abn_ctx* c = p->ctx;
  FitArgs a = phase_args(p, 0, w0, wn);
  if (early) {   // W == 1: the counter and the flag are the one window's
    a.quorum_words = early_words(p) + kEarlyCount;
    a.quorum = p->early.quorum;
  }
  if (timed) HIPCHK(c, hipEventRecord(p->ev[kEvFitA], st));
  if (int rc = launch_phase(p, 0, a, st, timed)) return rc;
  const SelectArgs s = select_args(p, w0, wn);
  if (timed) HIPCHK(c, hipEventRecord(p->ev[kEvSelect], st));
  if (int rc = launch_select(c, s, p->route.select_lds, st)) return rc;
  if (timed && !b_follows) HIPCHK(c, hipEventRecord(p->ev[kEvSelectEnd], st));
  return ABN_OK;
}

// Phase B (bootstraps) for windows [w0, w0+wn) on stream st.  timed: its first record is kEvFitB behind the selection
// of the same step (a_precedes), kEvFitBOwn where it runs on its own.
// A guarded launch (abn_plan_run with early bootstraps) stops when (*guard != 0) == guard_stop — the persistent kernel
// looks every guard_poll steps, the tail's resume launch at its entry — and counts in the words of `slot`.
struct PhaseGuard {
  const unsigned* word = nullptr;
  int stop = 0, poll = 0, slot = -1;
  bool ends_phase = true;   // a timed launch records kEvFitBEnd behind it (the early launch does not: the redo follows)
};
static int enqueue_phase_b(abn_plan* p, int w0, int wn, hipStream_t st, bool timed, bool a_precedes,
                           const PhaseGuard& guard = PhaseGuard{}) {
  abn_ctx* c = p->ctx;
  FitArgs a = phase_args(p, 1, w0, wn);
  a.guard = guard.word;
  a.guard_stop = guard.stop;
  a.guard_poll = guard.poll;
  if (timed) HIPCHK(c, hipEventRecord(p->ev[a_precedes ? kEvFitB : kEvFitBOwn], st));
  if (p->stream_b) {  // gather the bootstrap observations once per fit, then stream them
    double* dst = p->dstar.p + window_offsets(p, w0).boots * (size_t)p->N;
    const long long total = (long long)wn * p->B * p->N;
    const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 64LL * c->cus);
    hipLaunchKernelGGL(abn_make_dstar_kernel, dim3(blocks), dim3(256), 0, st, dst, a.pred, a.resid, a.idx, p->N,
                       (long long)p->B * p->N, total);
    HIPCHK(c, hipGetLastError());
    a.dmode = 2;
    a.D = dst;
  }
  if (int rc = launch_phase(p, 1, a, st, timed, guard.slot)) return rc;
  if (timed && guard.ends_phase) HIPCHK(c, hipEventRecord(p->ev[kEvFitBEnd], st));
  return ABN_OK;
}

// The head of a step: everything its launches need cleared, in one launch on the context's stream (abn_prepare.hpp).
// phase < 0: a whole step (abn_plan_run) — all of the plan's words, the redo slot, the early bootstraps' counters and flags
// and the status words included, the FIFO, and with `early` the redo's FIFO; phase 0 / 1: that phase's run on its own.
// What the list leaves clear is read off the list (prep_clean), and the record of the phases it serves is opened.
static int prepare_step(abn_plan* p, int phase, bool early) {
  const bool sweep = p->sweep_passes.p != nullptr;
  const size_t list = (size_t)p->W * (size_t)p->S;
  const bool whole_step = phase < 0;
  const PrepList l = whole_step ? prep_step(p->slice_cap, early, sweep, p->twopass_a && p->S > 0, list)
                                : prep_phase(phase, p->slice_cap, sweep, p->twopass_a, list);
  if (int rc = clear_ranges(p->ctx, l, prep_bases(p), p->ctx->stream)) return rc;
  p->clean = prep_clean(l, p->slice_cap, list);
  // the stream sweep's record (flag and pass counter per phase) is of the last run of each phase
  for (int ph = 0; ph < 2; ++ph)
    if (whole_step || ph == phase) p->rec[ph].sweep = false;
  return ABN_OK;
}

// The end of a step whose every launch has been enqueued: which phases ran, which records bound their spans (a phase
// that did not run keeps its own), and whether phase B was an early-bootstraps run.
static void end_step(abn_plan* p, bool ran_a, bool ran_b, bool early) {
  if (ran_a) {
    p->rec[0].ran = true;
    p->model_ready = true;
    p->select_span.end = ran_b ? kEvFitB : kEvSelectEnd;   // phase B's first record closes the selection where it follows
  }
  if (ran_b) {
    p->rec[1].ran = true;
    p->rec[1].span.begin = ran_a ? kEvFitB : kEvFitBOwn;
    p->early_rec.ran = early;
  }
}

// Window groups (run_step).  opts.window_groups > 1 cuts the plan into contiguous window groups that run A -> select -> B
// on their own HIP streams (a window's bootstraps need only that window's starts), forking from and joining
// back into the context's stream with events; results do not depend on the grouping and timing events are
// recorded for group 0.  Streams share a few in-order hardware queues (4 by default), so more than 4 groups
// serialise behind each other; see scripts/groups_bench.py for the measured effect.
static int ensure_fork_join(abn_plan* p, int streams) {
  abn_ctx* c = p->ctx;
  while ((int)c->side.size() < streams) {
    hipStream_t st = nullptr;
    HIPCHK(c, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    c->side.push_back(st);
  }
  if (!p->ev_fork) HIPCHK(c, hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
  while ((int)p->ev_join.size() < streams) {
    hipEvent_t e = nullptr;
    HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    p->ev_join.push_back(e);
  }
  return ABN_OK;
}

// One step, the same sequence for every entry point: the head's clears (prepare_step(prep)), then for each window group
// phase A with the selection (run_a) and phase B (run_b), then the record (end_step).  One group runs on the context's
// stream; more fork from it and join back into it.
static int run_step(abn_plan* p, int prep, bool run_a, bool run_b) {
  abn_ctx* c = p->ctx;
  // window groups need both phases: a phase on its own runs whole
  const int groups = run_a && run_b ? std::max(1, std::min(p->opt.window_groups, p->W)) : 1;
  const bool forked = groups > 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (forked)
    if (int rc = ensure_fork_join(p, groups)) return rc;
  if (int rc = prepare_step(p, prep, false)) return rc;
  if (forked) HIPCHK(c, hipEventRecord(p->ev_fork, c->stream));
  for (int g = 0; g < groups; ++g) {
    const int w0 = (int)((long long)p->W * g / groups), wn = (int)((long long)p->W * (g + 1) / groups) - w0;
    hipStream_t st = forked ? c->side[(size_t)g] : c->stream;
    if (forked) HIPCHK(c, hipStreamWaitEvent(st, p->ev_fork, 0));
    // groups share the plan's one queue: no persistent kernel; timing events are recorded for group 0
    if (run_a)
      if (int rc = enqueue_phase_a(p, w0, wn, st, g == 0, run_b)) return rc;
    if (run_b)
      if (int rc = enqueue_phase_b(p, w0, wn, st, g == 0, run_a)) return rc;
    if (forked) HIPCHK(c, hipEventRecord(p->ev_join[(size_t)g], st));
  }
  // Join only after every group has been enqueued: HIP multiplexes streams onto a few in-order hardware
  // queues, and a wait packet of the main stream placed between the launches would hold back whichever side
  // stream shares its queue (scripts/stream_overlap_test.hip: 10 ms instead of 5 ms for four 5 ms kernels).
  for (int g = 0; forked && g < groups; ++g) HIPCHK(c, hipStreamWaitEvent(c->stream, p->ev_join[(size_t)g], 0));
  end_step(p, run_a, run_b, false);
  return ABN_OK;
}

extern "C" int abn_plan_run_phase(abn_plan* p, int32_t phase) {
  if (!p) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = p->ctx;
  if (!p->windows_set) return set_err(c, ABN_ERR_STATE, "abn_plan_set_windows has not been called");
  if (phase != 0 && phase != 1) return set_err(c, ABN_ERR_INVALID_ARG, "phase must be 0 or 1");
  if (phase == 0 && p->S <= 0) return set_err(c, ABN_ERR_STATE, "plan has no starts");
  if (phase == 1 && p->B <= 0) return set_err(c, ABN_ERR_STATE, "plan has no bootstraps");
  if (phase == 1 && !p->model_ready) return set_err(c, ABN_ERR_STATE, "phase A has not run");
  return run_step(p, phase, phase == 0, phase == 1);
}

// Wavefront-steps between two looks of the early phase B at the miss word (a power of two; a step is ~2.7 us on C3, so a
// missed phase B stops within ~175 us).  Timed at 16 and at 64: 64 is 0.05 ms of a 3 ms step faster on a hit, three runs
// each against a spread of 0.013 (docs/experiments.md, "Early bootstraps"); tail mode polls every 64 as well.
constexpr int kGuardPoll = 64;

// abn_plan_run of a plan route_early_bootstraps admits.  No host synchronisation and no wait on a memory value: every
// launch is enqueued, and those that must not run find that out from the miss word at their entry.
//   main: prepare (every clear of the step, the redo's FIFO included) -> A pass 1 (ends at the quorum)
//         -> select over the finished starts -> fork
//   side: A resume (the parked starts) -> select over all starts (scratch) -> compare (raises miss) -> join
//   main: B + its tail (stop once miss is raised) -> wait for the join -> adopt the scratch selection
//         -> B + its tail again, in the redo slot (run only if miss is raised)
// The side work is enqueued before B and the join wait behind B's launches, for the reason given in run_step.
static int plan_run_early(abn_plan* p) {
  abn_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = ensure_fork_join(p, 1)) return rc;
  hipStream_t side = c->side[0];
  unsigned* ew = early_words(p);
  if (int rc = prepare_step(p, -1, true)) return rc;
  if (int rc = enqueue_phase_a(p, 0, p->W, c->stream, true, true, true)) return rc;
  HIPCHK(c, hipEventRecord(p->ev_fork, c->stream));
  HIPCHK(c, hipStreamWaitEvent(side, p->ev_fork, 0));
  {  // the stragglers: one workgroup per slot of their list (at most S - quorum can be running when the flag goes up)
    FitArgs a = phase_args(p, 0, 0, p->W);
    a.state = p->early_state.p;
    a.susp_list = p->early_list.p;
    a.susp_count = reinterpret_cast<int*>(ew + kEarlyParked);
    a.slice_status = ew + kEarlySink;
    a.skipped = p->skipped.p + kPhaseSkipped;
    if (int rc = launch_tail_resume(c, p->route, a, p->S - p->early.quorum, side)) return rc;
  }
  const SelectArgs to = select_args(p, 0, p->W);
  SelectArgs all = to;   // the same rule over all starts: the LSEs are the plan's, the choice goes to scratch
  all.model = p->sel_model.p;
  all.pred = p->sel_pred.p;
  all.resid = p->sel_resid.p;
  all.best_start = p->sel_best.p;
  if (int rc = launch_select(c, all, p->route.select_lds, side)) return rc;
  hipLaunchKernelGGL(abn_early_compare_kernel, dim3(1), dim3(kWave), 0, side, to.best_start, all.best_start, p->W, ew + kEarlyMiss);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(p->ev_join[0], side));
  PhaseGuard g;
  g.word = ew + kEarlyMiss;
  g.stop = 1;
  g.poll = kGuardPoll;
  g.ends_phase = false;
  if (int rc = enqueue_phase_b(p, 0, p->W, c->stream, true, true, g)) return rc;
  HIPCHK(c, hipStreamWaitEvent(c->stream, p->ev_join[0], 0));
  hipLaunchKernelGGL(abn_early_adopt_kernel, dim3(1), dim3(256), 0, c->stream, all, to);
  HIPCHK(c, hipGetLastError());
  g.stop = 0;
  g.poll = 0;
  g.slot = kSlotRedo;
  if (int rc = enqueue_phase_b(p, 0, p->W, c->stream, false, true, g)) return rc;
  HIPCHK(c, hipEventRecord(p->ev[kEvFitBEnd], c->stream));   // fit_boot: from the early launch to the end of the redo
  end_step(p, true, true, true);
  return ABN_OK;
}

static bool early_applies(const abn_plan* p) { return p->early.eligible && p->early_mode != 0; }

extern "C" int abn_plan_set_early_bootstraps(abn_plan* p, int32_t mode) {
  if (!p) return ABN_ERR_INVALID_ARG;
  if (mode != 0 && mode != 1) return set_err(p->ctx, ABN_ERR_INVALID_ARG, "early bootstraps: mode must be 0 (off) or 1 (auto)");
  p->early_mode = mode;
  return ABN_OK;
}

static int verify_persistent(abn_plan* p);

extern "C" int abn_plan_set_stream_sweep(abn_plan* p, int32_t mode) {
  if (!p) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = p->ctx;
  if (mode != 0 && mode != 1) return set_err(c, ABN_ERR_INVALID_ARG, "stream sweep: mode must be 0 (off) or 1 (on)");
  if (mode == 1 && !p->sweep_passes.p) {
    HIPCHK(c, hipSetDevice(c->device));
    PoolScope pool_scope(c);
    hipError_t e = p->sweep_passes.alloc(2);  // one counter per phase
    if (e != hipSuccess) return set_err(c, ABN_ERR_HIP, std::string("hipMalloc sweep_passes: ") + hipGetErrorString(e));
    PrepList l;   // both pass counters, outside a step: the memset form of the step's description
    l.add(kPrepSweep, 0, p->sweep_passes.bytes(), 0x00);
    if (int rc = clear_ranges(c, l, prep_bases(p), c->stream, false)) return rc;
  }
  p->sweep_mode = mode;
  return ABN_OK;
}

extern "C" int abn_plan_stream_sweep(abn_plan* p, int64_t* out4) {
  if (!p || !out4) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = p->ctx;
  unsigned long long passes[2] = {0, 0};
  if (p->sweep_passes.p) {
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = to_host(c, passes, p->sweep_passes)) return rc;
  }
  const int rc = verify_persistent(p);  // synchronises the stream
  out4[0] = p->sweep_mode;
  out4[1] = p->rec[0].sweep ? 1 : 0;
  out4[2] = p->rec[1].sweep ? 1 : 0;
  out4[3] = (int64_t)((p->rec[0].sweep ? passes[0] : 0) + (p->rec[1].sweep ? passes[1] : 0));
  return rc;
}

extern "C" int abn_plan_run(abn_plan* p) {
  if (!p) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = p->ctx;
  if (!p->windows_set) return set_err(c, ABN_ERR_STATE, "abn_plan_set_windows has not been called");
  if (early_applies(p)) return plan_run_early(p);
  const bool run_a = p->S > 0, run_b = p->B > 0;
  if (!run_a && !run_b) return ABN_OK;
  if (!run_a && !p->model_ready) return set_err(c, ABN_ERR_STATE, "phase A has not run");
  return run_step(p, run_a ? -1 : 1, run_a, run_b);   // with phase A: one clear for both phases
}

// A persistent launch must have finished every chain it was given: a lost FIFO entry or a chain that was parked and never
// taken up again would otherwise leave stale (or, in a bound buffer, uninitialised) rows in the tables.  Synchronises the
// stream.  Every entry point a caller can take results from runs this — abn_plan_sync (bind_raw / raw_device_ptr users:
// the torch.distributed shard runner), abn_plan_failed_windows, abn_plan_download, and through them abn_multi_sync /
// abn_multi_download.
static int verify_persistent(abn_plan* p) {
  abn_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  PlanWordsHost h{};
  if (p->rec[0].expected > 0 || p->rec[1].expected > 0 || p->early_rec.ran)
    if (int rc = fetch_words(p, h)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (p->early_rec.ran) {
    p->early_rec.parked = (int32_t)h.early[kEarlyParked];
    p->early_rec.miss = h.early[kEarlyMiss] != 0 ? 1 : 0;
  }
  for (int ph = 0; ph < 2; ++ph) {
    PhaseRecord& rec = p->rec[ph];
    if (rec.expected <= 0) continue;
    const unsigned* s = h.slice[phase_slot(p, ph, h)];
    rec.handed = (long long)s[kSliceHanded];
    if (s[kSliceError] != 0 || (long long)s[kSliceFinished] != rec.expected)
      return set_err(c, ABN_ERR_HIP, std::string("persistent fit launch of phase ") + (ph ? "B" : "A") + " finished " +
                                         std::to_string(s[kSliceFinished]) + " of " + std::to_string(rec.expected) +
                                         " chains (error word " + std::to_string(s[kSliceError]) + ", " + std::to_string(s[kSliceHanded]) +
                                         " handed to the speculative kernel, list length " + std::to_string(s[kSliceTailFill]) +
                                         "): results are incomplete");
  }
  return ABN_OK;
}

extern "C" int abn_plan_sync(abn_plan* p) {
  if (!p) return ABN_ERR_INVALID_ARG;
  return verify_persistent(p);
}

extern "C" int abn_plan_tail_handed(abn_plan* p, int64_t* out2) {
  if (!p || !out2) return ABN_ERR_INVALID_ARG;
  const int rc = verify_persistent(p);  // synchronises the stream and reads the counts of the last persistent launches
  for (int ph = 0; ph < 2; ++ph) out2[ph] = p->rec[ph].expected > 0 ? p->rec[ph].handed : 0;
  return rc;
}

extern "C" int abn_plan_early_bootstraps(abn_plan* p, int32_t* out4) {
  if (!p || !out4) return ABN_ERR_INVALID_ARG;
  const int rc = verify_persistent(p);  // synchronises the stream and reads the words of the last run
  out4[0] = p->early.eligible ? 1 : 0;
  out4[1] = p->early.eligible ? p->early.quorum : 0;
  out4[2] = p->early_rec.ran ? p->early_rec.parked : 0;
  out4[3] = p->early_rec.ran ? p->early_rec.miss : 0;
  return rc;
}

extern "C" int abn_plan_kernel_ms(abn_plan* p, double* ms3) {
  if (!p || !ms3) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const EventSpan span[3] = {p->rec[0].span, p->select_span, p->rec[1].span};  // fit_starts, select, fit_boot
  const bool ran[3] = {p->rec[0].ran, p->rec[0].ran, p->rec[1].ran};
  for (int k = 0; k < 3; ++k) {
    float ms = 0.f;
    if (ran[k]) HIPCHK(c, hipEventElapsedTime(&ms, p->ev[span[k].begin], p->ev[span[k].end]));
    ms3[k] = ms;
  }
  return ABN_OK;
}

extern "C" int abn_plan_raw_device_ptr(abn_plan* p, void** dev_ptr) {
  if (!p || !dev_ptr) return ABN_ERR_INVALID_ARG;
  *dev_ptr = p->raw;
  return ABN_OK;
}

extern "C" int abn_plan_bind_raw(abn_plan* p, void* dev_ptr) {
  if (!p) return ABN_ERR_INVALID_ARG;
  p->raw = dev_ptr ? (double*)dev_ptr : p->raw_own.p;
  return ABN_OK;
}

// The selection's verdict per window (best_start; -1: no finite start), for a plan whose phase A has run: read_verdict
// enqueues its copy on the context's stream — bs holds it once the caller has synchronised — and failed_windows counts
// the windows without a finite start (an empty bs: none).
static int read_verdict(const abn_plan* p, std::vector<int32_t>& bs) {
  bs.resize((size_t)p->W);
  return to_host(p->ctx, bs.data(), p->best_start);
}
static int32_t failed_windows(const std::vector<int32_t>& bs) {
  int32_t n = 0;
  for (int32_t b : bs) n += b < 0 ? 1 : 0;
  return n;
}

extern "C" int abn_plan_download(abn_plan* p, double* models, double* pred, double* resid, double* raw,
                                 abn_fit_info* info_a, abn_fit_info* info_b, int32_t* best_start) {
  if (!p) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = p->ctx;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t W = (size_t)p->W, B = (size_t)p->B;
  int rc;
  if ((rc = to_host(c, models, p->model)) || (rc = to_host(c, pred, p->pred)) || (rc = to_host(c, resid, p->resid)) ||
      (B && (rc = to_host(c, raw, p->raw, W * B * 7 * sizeof(double)))) || (p->S && (rc = to_host(c, info_a, p->infoA))) ||
      (B && (rc = to_host(c, info_b, p->infoB))))
    return rc;
  std::vector<int32_t> bs;
  if (p->rec[0].ran)  // the selection's verdict per window, whether or not the caller asked for it
    if ((rc = read_verdict(p, bs))) return rc;
  if ((rc = verify_persistent(p))) return rc;  // synchronises the stream
  if (best_start) {
    if (p->rec[0].ran) std::copy(bs.begin(), bs.end(), best_start);
    else std::fill(best_start, best_start + W, 0);  // model uploaded by the caller (abn_boot_model_run)
  }
  // every buffer has been filled; windows whose starts all ended non-finite carry NaN and best_start = -1
  if (failed_windows(bs) > 0)
    return set_err(c, ABN_ERR_NO_FINITE_FIT, "a window has no finite start (best_start = -1): its rows are NaN");
  return ABN_OK;
}

// src/analysis.rs:50-98 for every window of the table the plan currently writes (its own or the bound one), on the device
extern "C" int abn_plan_analyze(abn_plan* p, double* out, int32_t* first_bad) {
  if (!p) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = p->ctx;
  if (!out) return set_err(c, ABN_ERR_INVALID_ARG, "null out");
  if (!p->rec[1].ran || p->B <= 0) return set_err(c, ABN_ERR_STATE, "phase B has not run: there is no bootstrap table");
  if (int rc = verify_persistent(p)) return rc;  // synchronises the stream
  return analyze_device_table(c, p->raw, p->W, p->B, out, first_bad);
}

extern "C" int abn_plan_failed_windows(abn_plan* p, int32_t* n_failed) {
  if (!p || !n_failed) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = p->ctx;
  *n_failed = 0;
  if (!p->rec[0].ran) return verify_persistent(p);
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<int32_t> bs;
  if (int rc = read_verdict(p, bs)) return rc;
  if (int rc = verify_persistent(p)) return rc;  // synchronises the stream
  *n_failed = failed_windows(bs);
  return ABN_OK;
}

extern "C" int abn_plan_counters(abn_plan* p, int64_t* out5) {
  if (!p || !out5) return ABN_ERR_INVALID_ARG;
  abn_ctx* c = p->ctx;
  out5[0] = out5[1] = out5[2] = out5[3] = out5[4] = 0;
  HIPCHK(c, hipSetDevice(c->device));
  const DevBuf<FitInfoDev>* info[2] = {&p->infoA, &p->infoB};
  std::vector<FitInfoDev> h[2];
  PlanWordsHost wd{};
  for (int ph = 0; ph < 2; ++ph) {
    if (!p->rec[ph].ran || !info[ph]->n) continue;
    h[ph].resize(info[ph]->n);
    if (int rc = to_host(c, h[ph].data(), *info[ph])) return rc;
  }
  if (int rc = fetch_words(p, wd)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int ph = 0; ph < 2; ++ph) {
    if (h[ph].empty()) continue;
    for (const auto& f : h[ph]) {
      out5[0] += 1;
      out5[1] += f.evals;
      out5[2] += f.iters;
    }
    out5[3 + ph] = (int64_t)wd.phase[phase_slot(p, ph, wd)][kPhaseSkipped];
  }
  return ABN_OK;
}

#ifdef ABN_STAMPS
// diagnostic build only: run phase A with in-kernel stamps, return the 8 cycle sums of chain 0
static int debug_stamps(abn_plan* p, unsigned long long* out8, bool spec) {
  abn_ctx* c = p->ctx;
  DevBuf<unsigned long long> d;
  HIPCHK(c, d.alloc(8));
  HIPCHK(c, hipMemsetAsync(d.p, 0, 64, c->stream));
  FitArgs a = phase_args(p, 0, 0, p->W);
  a.dbg = d.p;
  int rc = launch_fit(c, p->route, PhaseRoute{spec, p->route.lanes, false}, a, LaunchOffer{}, c->stream);
  if (rc) return rc;
  if ((rc = to_host(c, out8, d.p, 64))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}
extern "C" int abn_plan_debug_stamps(abn_plan* p, unsigned long long* out8) { return debug_stamps(p, out8, false); }
// the same for the speculative three-wavefront kernel (wavefront 0 of chain 0; out8[7] = iterations)
extern "C" int abn_plan_debug_stamps_spec(abn_plan* p, unsigned long long* out8) { return debug_stamps(p, out8, true); }
#endif

extern "C" int abn_plan_last_kernels(abn_plan* p, int32_t* out4) {
  if (!p || !out4) return ABN_ERR_INVALID_ARG;
  for (int ph = 0; ph < 2; ++ph) {
    out4[2 * ph] = p->rec[ph].kind;
    out4[2 * ph + 1] = p->rec[ph].lanes;
  }
  return ABN_OK;
}

extern "C" int abn_plan_device_bytes(abn_plan* p, int64_t* bytes) {
  if (!p || !bytes) return ABN_ERR_INVALID_ARG;
  size_t t = 0;
  t += p->D.bytes() + p->pred.bytes() + p->resid.bytes() + p->p_uu.bytes() + p->eqp.bytes() + p->eqp_w.bytes();
  t += p->simplexA.bytes() + p->bestA.bytes() + p->model.bytes() + p->lse.bytes() + p->bestB.bytes();
  t += p->raw_own.bytes() + p->infoA.bytes() + p->infoB.bytes() + p->best_start.bytes() + p->idx.bytes();
  t += p->dstar.bytes() + p->nm_state.bytes() + p->susp_list.bytes() + p->skipped.bytes() + p->slice_buf.bytes();
  t += p->wid.bytes() + p->early_state.bytes() + p->early_list.bytes() + p->sel_model.bytes() + p->sel_pred.bytes();
  t += p->sel_resid.bytes() + p->sel_best.bytes() + p->sweep_passes.bytes();
  t += p->dtopo.tri.bytes() + p->dtopo.tid.bytes();
  *bytes = (int64_t)t;
  return ABN_OK;
}

// ------------------------------------------------------------------------------------------------
// (2) ab_neutral::run and (3) boot_model::run on host buffers
// ------------------------------------------------------------------------------------------------
static void split_pedigree(const double* ped, int n, std::vector<double>& gens, std::vector<double>& d) {
  gens.resize((size_t)n * 3);
  d = column3(ped, n);
  for (size_t i = 0; i < (size_t)n; ++i) std::copy(ped + i * 4, ped + i * 4 + 3, gens.begin() + i * 3);
}

extern "C" int abn_ab_neutral_run(abn_ctx* c, const abn_options* opts, const double* pedigree, int32_t n_rows,
                                  double p0uu, double eqp, double eqp_weight, int32_t n_starts, double* model,
                                  double* pred, double* resid, double* all_models, abn_fit_info* info, double* lse) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (!pedigree || n_rows <= 0 || n_starts <= 0 || !model || !pred || !resid)
    return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  std::vector<double> gens, d;
  split_pedigree(pedigree, n_rows, gens, d);
  abn_plan* p = nullptr;
  int rc = abn_plan_create(c, opts, gens.data(), n_rows, 1, n_starts, 0, 0, 0, &p);
  if (rc) return rc;
  rc = abn_plan_set_windows(p, d.data(), &p0uu, &eqp, &eqp_weight);
  if (!rc) rc = abn_plan_run_phase(p, 0);
  // the optional outputs, on the stream behind phase A: abn_plan_download synchronises it
  if (!rc) rc = to_host(c, all_models, p->bestA);
  if (!rc) rc = to_host(c, lse, p->lse);
  int32_t best = -1;
  bool no_fit = false;
  if (!rc) {
    rc = abn_plan_download(p, model, pred, resid, nullptr, info, nullptr, &best);
    if (rc == ABN_ERR_NO_FINITE_FIT) {  // buffers are filled (NaN model); report once the plan is gone
      no_fit = true;
      rc = ABN_OK;
    }
  }
  abn_plan_destroy(p);
  if (!rc && (no_fit || best < 0)) rc = set_err(c, ABN_ERR_NO_FINITE_FIT, abn_status_string(ABN_ERR_NO_FINITE_FIT));
  return rc;
}

extern "C" int abn_boot_model_run(abn_ctx* c, const abn_options* opts, const double* pedigree, int32_t n_rows,
                                  const double* model, const double* pred, const double* resid, double p0uu,
                                  double eqp, double eqp_weight, int32_t n_boot, double* raw, abn_fit_info* info) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (!pedigree || n_rows <= 0 || n_boot <= 0 || !model || !pred || !resid || !raw)
    return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  std::vector<double> gens, d;
  split_pedigree(pedigree, n_rows, gens, d);
  abn_plan* p = nullptr;
  int rc = abn_plan_create(c, opts, gens.data(), n_rows, 1, 0, n_boot, 0, 0, &p);
  if (rc) return rc;
  rc = plan_upload_model(p, model, pred, resid, &p0uu, &eqp, &eqp_weight);
  if (!rc) rc = abn_plan_run_phase(p, 1);
  if (!rc) rc = abn_plan_download(p, nullptr, nullptr, nullptr, raw, nullptr, info, nullptr);
  abn_plan_destroy(p);
  return rc;
}
