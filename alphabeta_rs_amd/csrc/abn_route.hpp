// The launch policy of the fit path, and nothing else: which kernel instantiation runs, with which grid, LDS and reduction
// tree, for a pedigree, its resolved options and a number of chains.  Pure host arithmetic on plain integers — no context,
// no launch arguments, no HIP, no allocation — so that the same code decides in libabneutral_hip.so (abn_api.hip's launchers
// execute what it returns, for the one-shot entries and for abn_plan.hip) and answers on a machine without a GPU (host/host_capi.cpp: abh_route_*).
//
// Three levels, each one function returning a plain struct:
//   route_pedigree   N, K, T, lanes_per_chain, strict order  -> lanes, tree, resident or streamed, what the pedigree admits
//   route_phase      + phase A / B, the plan's chains, CUs   -> speculative, a wavefront per chain, or packed
//   route_launch     + what the caller offers                -> instantiation key, grid, block, LDS, stride, tree, quantum, tail
// A decision is a function of the pedigree and the options where results depend on it (the tree: DESIGN.md) and of the
// size of the launch only where they do not (the kernel).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>

#include "../../include/abneutral.h"
#include "abn_constants.hpp"

namespace abn {

// ------------------------------------------------------------------------------------------------
// thresholds (measured; the totals in the comments are the MI355X's: 256 CUs)
// ------------------------------------------------------------------------------------------------
constexpr size_t kDefaultDynLds = 64 * 1024;   // what a launch may ask for without opting in
constexpr size_t kMaxDynLds = 160 * 1024;      // gfx950: the whole LDS of a CU, for the one-chain-per-workgroup kernels
// A workgroup with one chain (stream-mode fits, selection, 64-lane cost) may need more than 64 KiB for pedigrees with
// thousands of distinct triples: the launcher opts the kernel in (hipFuncAttributeMaxDynamicSharedMemorySize).
constexpr size_t lds_limit(int lanes) { return lanes == kWave ? kMaxDynLds : kDefaultDynLds; }
constexpr size_t kLdsResidentMax = 40 * 1024;
// Launch geometry in wavefronts (or chains) PER CU.
#ifndef ABN_PERSIST_WAVES_PER_CU
#define ABN_PERSIST_WAVES_PER_CU 12
#endif
constexpr long long kPersistWavesPerCu = ABN_PERSIST_WAVES_PER_CU;  // a persistent launch: 3 per SIMD x 4 SIMDs (3072)
// A launch that would just about fill the resident wavefronts (2048 < wavefronts <= 3072: C3's 10 000 bootstraps are 2500)
// runs persistent on 2048 of them instead: the last fifth of the chains waits in the queue, finished groups refill and
// time slicing evens out the tail (C3 phase B 2.58 -> 2.44 ms; same box: 2.61 -> 2.53 ms, 1792 / 2304 wavefronts 2.71 /
// 2.82 ms; profiles/r03_persist_waves_sweep.txt)
#ifndef ABN_PERSIST_WAVES_SMALL_PER_CU
#define ABN_PERSIST_WAVES_SMALL_PER_CU 8
#endif
constexpr long long kPersistWavesSmallPerCu = ABN_PERSIST_WAVES_SMALL_PER_CU;
constexpr long long persist_waves(int cus) { return kPersistWavesPerCu * cus; }
constexpr long long persist_waves_small(int cus) { return kPersistWavesSmallPerCu * cus; }
constexpr long long persist_waves_for(int cus, long long blocks) {
  return blocks > persist_waves(cus) ? persist_waves(cus) : persist_waves_small(cus);
}
#ifndef ABN_PHASE_A_SPEC_PER_CU
#define ABN_PHASE_A_SPEC_PER_CU 4
#endif
constexpr long long kPhaseASpecPerCu = ABN_PHASE_A_SPEC_PER_CU;  // chains per CU abn_fit_spec_kernel keeps resident at up to two rows per lane (spec_max_chains)
constexpr long long kPhaseAWidePerCu = 24;                      // ... and up to which phase A uses one wavefront per chain (6144)
// Time slicing of persistent launches (FitArgs::quantum): evaluations a chain runs before it yields to waiting chains.
#ifndef ABN_QUANTUM
#define ABN_QUANTUM 256
#endif
constexpr int kQuantum = ABN_QUANTUM;
constexpr size_t kSliceStateMax = (size_t)256 << 20;  // bytes of parked state (kStateDoubles per chain of the launch)
constexpr int kPhaseACap = 1000;  // first-pass iteration cap of the two-pass phase A
constexpr long long kTwoPassChains = 4096;  // ... which needs more start chains than this
constexpr size_t kLdsTargetPerBlock = 20 * 1024;
constexpr const char* kLdsRefusal = "pedigree needs more LDS per workgroup than supported (T or K too large)";

// ------------------------------------------------------------------------------------------------
// footprints, in doubles per chain (each stated here once)
// ------------------------------------------------------------------------------------------------
// the topology's scratch stride: power table, dt1t2 per triple (KP = K rounded up to even), 4 per-chain constants
constexpr int scratch_stride(int tp, int kp) { return kPw * tp + kp + 4; }
// Doubles a chain's LDS region holds beyond the scratch stride when its pedigree is resident: the observations, the triple
// list of the K distinct triples (even: 16-byte aligned chains for load_matrix) and, in strict order, the rows' terms.
constexpr int resident_extra(int n, int k, int strict) {
  return ((n + 1) & ~1) + (((k + 1) / 2 + 1) & ~1) + (strict ? ((n + 1) & ~1) : 0);
}
// the speculative kernel's evaluation wavefronts: observations (+ strict order: the rows' terms), no triple list
constexpr int spec_extra(int n, int strict) { return ((n + 1) & ~1) * (strict ? 2 : 1); }
constexpr size_t spec_lds(int chain_stride, int n, int strict) {
  return (3 * (size_t)(chain_stride + spec_extra(n, strict)) + kSpecCommDoubles) * sizeof(double);
}
// a streamed chain: the scratch, plus one chunk of terms in strict order
constexpr int stream_stride(int chain_stride, int lanes, int strict) {
  return chain_stride + (strict ? kStrictRowsPerLane * lanes : 0);
}
// a streamed chain of abn_sweep_kernel: the scratch, plus two more dt tables (reflection, expansion and contraction each
// have their own; the power table is shared)
constexpr int sweep_stride(int chain_stride, int kp) { return chain_stride + 2 * kp; }
// selection kernels (one model per workgroup): power table, dt1t2, one chunk of terms
constexpr size_t select_lds(int tp, int kp) { return ((size_t)kPw * tp + kp + kSelChunk) * sizeof(double); }

// Rows per lane of a resident kernel (its RMAX template argument) by rows alone; 0: stream mode.
constexpr int pick_rmax(int n, int lanes) {
  const int per = (n + lanes - 1) / lanes;
  if (per <= 1) return 1;
  if (per <= 2) return 2;
  if (per <= 4) return 4;
  if (per <= 8) return 8;
  // 512 < N <= 1024: still LDS-resident with one wavefront per chain (scripts/n_sweep.py, N = 820, 2000 bootstraps:
  // 5.25 -> 4.0 ms; 32 rows per lane with the triple ids in LDS gained nothing over streaming: not kept)
  if (per <= 16 && lanes == kWave) return 16;
  return 0;
}
// ... and by the one residency footprint: a workgroup's 64 / lanes chains within kLdsResidentMax.  Every decision taken
// before a launch (plan, tree, kernel choice) and the launch itself ask this, so that what is decided is what runs.
constexpr int resident_rows(int n, int k, int chain_stride, int lanes, int strict) {
  const bool fits = (size_t)(kWave / lanes) * (size_t)(chain_stride + resident_extra(n, k, strict)) * sizeof(double) <= kLdsResidentMax;
  return fits ? pick_rmax(n, lanes) : 0;
}

// Lanes of a wavefront per chain.  Auto: by pedigree rows, then widened until the workgroup's LDS
// (64/G chains x chain_stride doubles) leaves room for >= 8 workgroups per CU (160 KiB LDS).
constexpr int pick_lanes(int n, int requested, int chain_stride) {
  if (requested == 8 || requested == 16 || requested == 32 || requested == 64) return requested;
  int g = 64;
  if (n <= 32) g = 8;
  else if (n <= 128) g = 16;
  else if (n <= 256) g = 32;
  const size_t per_chain = ((size_t)chain_stride + (size_t)n) * sizeof(double);  // scratch + resident observations
  while (g < 64 && (size_t)(kWave / g) * per_chain > kLdsTargetPerBlock) g *= 2;
  return g;
}

// ------------------------------------------------------------------------------------------------
// the instantiation key: what tests/_kernel_matrix.py decodes from the mangled names
// ------------------------------------------------------------------------------------------------
enum KernelFamily { kFamFit = 0, kFamRefill = 1, kFamSpec = 2, kFamCost = 3, kFamSweep = 4 };
struct KernelKey {
  int family;  // abn_fit_kernel<G, R, TP, STRICT>, abn_fit_refill_kernel<G, R>, abn_fit_spec_kernel<R, STRICT, RESUME>, abn_cost_kernel<G>,
               // abn_sweep_kernel<R> (G = 64; R: 0 its deep loop, -1 its pair loop)
  int G;       // lanes per chain (speculative: 64)
  int R;       // rows per lane; fit: 0 the deep stream loop, -1 the pair-loop stream variant; cost: 0
  bool tp, strict, resume;
};
constexpr bool operator==(const KernelKey& a, const KernelKey& b) {
  return a.family == b.family && a.G == b.G && a.R == b.R && a.tp == b.tp && a.strict == b.strict && a.resume == b.resume;
}

// ------------------------------------------------------------------------------------------------
// pedigree level: N rows, K distinct triples, largest generation T; lanes_per_chain as requested (0: auto) and the
// summation order resolved to 0 / 1
// ------------------------------------------------------------------------------------------------
struct PedigreeRoute {
  int n, k, tp, kp, chain_stride;  // chain_stride: the scratch stride (what FitArgs / CostArgs carry before a launch)
  int requested, strict;
  int lanes;          // of the packed (throughput) kernels
  // The residual reduction tree (FitArgs::tree; abn_fit_info.lanes).  Auto lanes and the pedigree LDS-resident: the
  // canonical 64-accumulator tree, which every kernel — packed, one wavefront per chain, four wavefronts per chain —
  // runs at its native cost.  Streamed pedigrees and explicit lane counts: one accumulator per lane of the packed
  // kernel.  Strict order: 1 (serial row order, no tree).
  int tree;
  int reported_tree;  // abn_reduction_tree: `tree`, streamed pedigrees marked lanes | (kStreamVec - 1) << 8
  bool streams;       // the packed kernels stream this pedigree
  bool wide_ok;       // a wavefront per chain computes the pedigree's tree
  bool spec_ok;       // ... and so does the speculative kernel (resident observations: not FitArgs::dmode 2)
  int spec_rows;      // its RMAX: rows per lane at 64 lanes, at most 8
  int cost_lanes, cost_tree;  // abn_cost_batch: abn_cost_kernel<cost_lanes>
  size_t cost_lds, select_lds;
  const char* refusal;         // abn_plan_create: nullptr, or why no plan can run this pedigree
  const char* cost_refusal;    // abn_cost_batch
  const char* select_refusal;  // abn_select_best
};

inline PedigreeRoute route_pedigree(int n, int k, int t, int requested, int strict) {
  PedigreeRoute p{};
  p.n = n;
  p.k = k;
  p.tp = t + 1;
  p.kp = (k + 1) & ~1;
  p.chain_stride = scratch_stride(p.tp, p.kp);
  p.requested = requested;
  p.strict = strict ? 1 : 0;
  p.lanes = pick_lanes(n, requested, p.chain_stride);
  p.streams = resident_rows(n, k, p.chain_stride, p.lanes, p.strict) == 0;
  p.tree = p.strict ? 1 : (requested != 0 || p.streams) ? p.lanes : kTreeCanon;
  p.reported_tree = (!p.strict && p.streams) ? (p.lanes | ((kStreamVec - 1) << 8)) : p.tree;
  // a wavefront per chain runs the canonical tree (or, strict order, the serial sum) whenever the pedigree is
  // LDS-resident at 64 lanes per chain; an explicit lanes_per_chain tree only when it IS 64 lanes
  p.wide_ok = (!p.strict && p.tree != kTreeCanon) ? p.tree == kWave
                                                   : resident_rows(n, k, p.chain_stride, kWave, p.strict) != 0;
  // Speculative kernel (three evaluation wavefronts + a bookkeeping wavefront per chain): resident mode with one
  // wavefront per candidate only, up to 8 rows per lane (16: the plain resident kernel), its footprint resident
  const int r64 = pick_rmax(n, kWave);
  p.spec_rows = r64 == 1 || r64 == 2 || r64 == 4 ? r64 : 8;
  p.spec_ok = r64 != 0 && r64 <= 8 && p.wide_ok && spec_lds(p.chain_stride, n, p.strict) <= kLdsResidentMax;
  // the cost batch sums with the pedigree's tree; strict order: one wavefront per candidate, terms in chunks
  p.cost_lanes = p.strict ? kWave : p.lanes;
  p.cost_tree = p.strict ? kWave : p.tree;
  p.cost_lds = ((size_t)(kWave / p.cost_lanes) * p.chain_stride + (p.strict ? kSelChunk : 0)) * sizeof(double);
  p.select_lds = select_lds(p.tp, p.kp);
  // A plan is refused at abn_plan_create, not at its first run: by the footprint of a streamed launch (resident launches
  // stay below kLdsResidentMax by construction) and by one chain's scratch next to a selection chunk.
  if ((size_t)(kWave / p.lanes) * stream_stride(p.chain_stride, p.lanes, p.strict) * sizeof(double) > lds_limit(p.lanes) ||
      ((size_t)p.chain_stride + kSelChunk) * sizeof(double) > kMaxDynLds)
    p.refusal = kLdsRefusal;
  if (p.cost_lds > lds_limit(p.cost_lanes)) p.cost_refusal = "pedigree needs more LDS than supported";
  if (p.select_lds > kMaxDynLds) p.select_refusal = "pedigree needs more LDS than supported";
  return p;
}

// ------------------------------------------------------------------------------------------------
// phase level: speculative, a wavefront per chain, or packed — by the size of the PLAN's phase (windows x starts or
// bootstraps, also when a window group launches its share), so that a plan's groups all take the same kernel
// ------------------------------------------------------------------------------------------------
// Chains up to which the speculative kernel is used.  What the GPU holds at once: four workgroups per CU for pedigrees of up
// to two rows per lane (1024 chains on the MI355X), three beyond (768); workgroups beyond that start as earlier ones end.
// Phase B (bootstrap chains: similar lengths) up to 1.5 x / 1 x of that; phase A (start chains from random points: lengths
// differ several-fold, so the queue behind the resident chains drains into slots that free early) up to 4 x / 2.7 x.
// Speculative / one wavefront per chain / packed, ms (scripts/b_kernel_sweep.py, scripts/a_kernel_sweep.py,
// profiles/r04_b_kernel_sweep.txt, r04_a_kernel_sweep.txt):
//   phase B, C3 topology: 1000 chains 0.76 / 1.03 / 1.60, 1500: 1.04 / 1.15 / 1.16, 2000: 1.28 / 1.31 / 1.31, 3000: 1.70 / 1.49 / 1.48;
//            6-row pedigree 1500: 1.44 / 1.95 / 1.95, 3000: 1.95 / 2.43 / 2.26; 351-row pedigree 500: 1.21 / 1.95 / 1.95, 1000: 2.14 / 1.97 / 1.96
//   phase A, C3 topology: 1000 chains 1.89 / 2.94 / 4.80, 2000: 2.71 / 3.31 / 4.94, 3000: 3.45 / 3.67 / 5.06, 4000: 4.21 / 4.40 / 6.13,
//            5000: 5.10 / 5.16 / 6.46, 6000: 6.15 / 5.75 / 6.43; 351-row pedigree 1000: 3.25 / 3.77 / 3.78, 2000: 6.11 / 6.43 / 6.31, 3000: 6.30 / 6.55 / 6.54
constexpr long long spec_max_chains(int cus, int n_rows, int phase) {
  const long long mx = kPhaseASpecPerCu * cus;   // 1024
  const bool small = pick_rmax(n_rows, kWave) <= 2;
  if (phase == 0) return small ? mx * 4 : mx * 2;
  return small ? mx * 3 / 2 : mx * 3 / 4;
}
// Phase A with many chains when the repetitions of stuck fits must be executed (no_fixed_point_skip): 7 % of
// random starts run into argmin's fixed point and repeat it up to iteration 10000; dispatched late in one launch
// such a chain runs alone for tens of milliseconds.  Two passes: every chain for at most kPhaseACap iterations,
// then the unfinished ones, compacted, all resident at once.  With the default skip those chains end at once and
// one pass is faster (metaprofile shape, 30000 start chains: 14.6 ms against 18.3 ms).
constexpr bool plan_two_pass(long long start_chains, int max_iters_start, int no_fixed_point_skip, int shrink, int strict) {
  return start_chains > kTwoPassChains && max_iters_start > kPhaseACap && no_fixed_point_skip != 0 && shrink == 0 && !strict;
}

struct PhaseRoute {
  bool spec;      // abn_fit_spec_kernel: four wavefronts per chain
  int lanes;      // otherwise abn_fit_kernel / abn_fit_refill_kernel at this many lanes per chain (64: a wavefront per chain)
  bool two_pass;  // phase A of a whole plan: launch pass 1, then pass 2 (LaunchOffer::pass)
};

// phase 0 = A (starts), 1 = B (bootstraps); dmode: FitArgs::dmode of the launch (2: streamed bootstrap observations);
// whole: the launch covers every window of the plan; two_pass: plan_two_pass of the plan;
// force: nullptr, or "spec" | "wide" | "packed" (ABN_MEASUREMENT_KNOBS builds: scripts/a_kernel_sweep.py, b_kernel_sweep.py)
inline PhaseRoute route_phase(const PedigreeRoute& p, int phase, long long plan_chains, int cus, int dmode, bool whole,
                              bool two_pass, const char* force = nullptr) {
  const bool can_wide = p.requested == 0 && dmode != 2 && p.wide_ok;
  const bool can_spec = can_wide && p.spec_ok;
  PhaseRoute r{false, p.lanes, false};
  // Few chains: latency-bound -> three wavefronts per chain evaluate reflection / expansion / contraction at once, a
  // fourth keeps the simplex and prepares the next candidates meanwhile.  Beyond that a wavefront per chain still beats
  // packing several chains into one:
  //   phase A while its chains fit the machine about twice over (3 wavefronts x 1024 SIMDs; scripts/phase_a_sweep.py, C3
  //   topology: 1000 chains 2.6 / 3.2 / 4.6 ms for speculative / 64 lanes / 16 lanes, 1500 chains 4.2 / 3.4 / 4.8; 4000
  //   chains - / 4.6 / 5.9 ms; 8000 chains - / 7.7 / 7.0 ms);
  //   phase B up to 192 chains per packed lane (3072 for the 16-lane kernels; scripts/b_kernel_sweep.py, C3 topology: 2000
  //   bootstraps 1.36 ms against 1.74 ms packed and 1.81 ms speculative; 4000: 1.99 against 1.75; bundled 6-row pedigree,
  //   8 lanes: 2000 bootstraps 1.98 against 1.90).
  // The reduction tree stays the pedigree's whichever kernel runs: results do not depend on the size of the launch, hence
  // not on how a job is sharded over GPUs.
  r.spec = can_spec && plan_chains <= spec_max_chains(cus, p.n, phase);
  if (!r.spec && can_wide && plan_chains <= (phase == 0 ? kPhaseAWidePerCu * cus : (3LL * cus / 4) * p.lanes)) r.lanes = kWave;
  if (force && !strcmp(force, "spec")) r.spec = can_spec;
  if (force && !strcmp(force, "wide")) r = {false, can_wide ? kWave : p.lanes, false};
  if (force && !strcmp(force, "packed")) r = {false, p.lanes, false};
  if (r.spec) r.lanes = kWave;
  r.two_pass = !r.spec && phase == 0 && whole && two_pass;
  return r;
}

// ------------------------------------------------------------------------------------------------
// launch level
// ------------------------------------------------------------------------------------------------
struct LaunchOffer {
  bool queue = false;    // a zeroed chain counter (FitArgs::queue): the launch may be persistent
  bool parking = false;  // ... and state, FIFO, tail list and status words: it may time-slice and hand its tail over
  int pass = 0;          // two-pass phase A: 1 = every chain up to kPhaseACap iterations, 2 = the parked ones to the end
  bool sweep = false;    // opt-in (abn_plan_set_stream_sweep): a streamed launch of one wavefront per chain may take abn_sweep_kernel
};

struct LaunchRoute {
  int status;          // ABN_OK, or the error to return with `error` as its text
  const char* error;
  int kind;            // ABN_KERNEL_* (NONE: no chains, nothing to launch)
  KernelKey key;
  unsigned grid, block;
  size_t lds;
  int chain_stride;    // as launched: the scratch stride plus what the variant keeps next to it
  int tree;
  int quantum;         // persistent launches: evaluations per time slice, 0 = no slicing
  int tail_cap;        // > 0: chains the launch may hand to route_tail_resume's launch, which then follows it
};

// More wavefronts than the GPU should hold at once and several chains per wavefront: the persistent kernel, whose groups
// take the next chain from a queue when their fit ends.  By size alone: abn_plan_create sizes the parking buffers of a
// plan by this, route_launch adds what the launch itself must be (resident, one pass, a queue offered).
constexpr bool persistent_by_size(int lanes, long long chains, int cus) {
  const int ng = kWave / lanes;
  return ng > 1 && (chains + ng - 1) / ng > persist_waves_small(cus);
}
// chains a whole plan's launches may park (0: no time slicing): those of its larger phase, within kSliceStateMax of state
constexpr size_t plan_sliced_chains(const PedigreeRoute& p, size_t chains, int cus, int window_groups) {
  return kQuantum > 0 && persistent_by_size(p.lanes, (long long)chains, cus) && chains * kStateDoubles * sizeof(double) <= kSliceStateMax &&
                 chains < (1u << 27) && window_groups <= 1
             ? chains : 0;
}
// Tail hand-over (FitArgs::tail_cap): the last chains of a time-sliced launch finish on four wavefronts each instead of one
// by one on an emptying GPU at the packed kernel's step time (metaprofile shape, phase A: 12 of 17 ms were such a tail).
// As many as abn_fit_spec_kernel keeps resident (four per CU at up to two rows per lane), twice that behind the deep queues
// of the 12-wavefronts-per-CU geometry, where the later workgroups start as the first end (scripts/tail_sweep.sh,
// profiles/r04_tail_sweep.txt: C3 is best at 1024, the C4 shard and the metaprofile shape at 2048-3072: +3 % / +2 %).
// Needs the canonical tree and the speculative kernel to apply to the pedigree.
constexpr int tail_cap_for(const PedigreeRoute& p, long long blocks, int cus) {
  if (p.tree != kTreeCanon || !p.spec_ok) return 0;
  return (int)((pick_rmax(p.n, kWave) <= 2 ? (blocks == persist_waves(cus) ? 8LL : 4LL) : 2LL) * cus);
}

inline LaunchRoute refuse(const char* why) {
  LaunchRoute r{};
  r.status = ABN_ERR_INVALID_ARG;
  r.error = why;
  return r;
}

// the speculative kernel: one workgroup of four wavefronts per chain.  resume: the parked tail of a persistent launch,
// one workgroup per slot of the tail list (those beyond its fill count leave at once)
inline LaunchRoute route_spec(const PedigreeRoute& p, long long chains, bool resume) {
  LaunchRoute r{};
  if (chains <= 0) return r;
  if (!p.spec_ok) return refuse("internal: the speculative kernel does not apply to this pedigree");
  r.kind = ABN_KERNEL_SPECULATIVE;
  r.key = {kFamSpec, kWave, p.spec_rows, false, p.strict != 0, resume};
  r.grid = (unsigned)chains;
  r.block = 4 * kWave;
  r.chain_stride = p.chain_stride + spec_extra(p.n, p.strict);
  r.lds = spec_lds(p.chain_stride, p.n, p.strict);
  r.tree = p.strict ? 1 : kTreeCanon;
  return r;
}
inline LaunchRoute route_tail_resume(const PedigreeRoute& p, int tail_cap) { return route_spec(p, tail_cap, true); }

inline LaunchRoute route_launch(const PedigreeRoute& p, const PhaseRoute& ph, long long chains, int cus, const LaunchOffer& o) {
  if (ph.spec) return route_spec(p, chains, false);
  LaunchRoute r{};
  if (chains <= 0) return r;
  const int lanes = ph.lanes, ng = kWave / lanes;
  if (p.strict && o.pass != 0) return refuse("internal: strict order has no two-pass variant");
  // one accumulator per lane means the lanes of THIS launch (a wavefront per chain admits such a tree only at 64)
  r.tree = p.strict ? 1 : p.tree == kTreeCanon ? kTreeCanon : lanes;
  int rows = resident_rows(p.n, p.k, p.chain_stride, lanes, p.strict);
  if (rows > 0) {
    r.chain_stride = p.chain_stride + resident_extra(p.n, p.k, p.strict);
  } else {
    if (r.tree == kTreeCanon) return refuse("internal: the canonical tree needs an LDS-resident pedigree");
    r.chain_stride = stream_stride(p.chain_stride, lanes, p.strict);
    // rows shorter than one trip of the deep loop (kStreamBlocks x 4 rows x lanes) use the pair-loop variant; strict
    // order has one stream variant (chunks of 8 G rows)
    rows = (!p.strict && p.n < 2 * kStreamBlocks * kStreamVec * lanes) ? -1 : 0;
    // Opt-in: one pass over the rows per iteration (abn_fit_sweep.hpp).  One wavefront per chain, tree order, one pass, and
    // its larger footprint within the limit; every other launch keeps the route it has without the offer.  Same tree, same bits.
    if (o.sweep && lanes == kWave && !p.strict && o.pass == 0) {
      const int stride = sweep_stride(p.chain_stride, p.kp);
      const size_t lds = (size_t)stride * sizeof(double);
      if (lds <= lds_limit(lanes) && chains <= 0x7fffffffLL) {
        r.kind = ABN_KERNEL_STREAM_SWEEP;
        r.key = {kFamSweep, kWave, p.n < kSweepBlocks * kStreamVec * kWave ? -1 : 0, false, false, false};
        r.chain_stride = stride;
        r.lds = lds;
        r.grid = (unsigned)chains;
        r.block = kWave;
        return r;
      }
    }
  }
  r.lds = (size_t)ng * (size_t)r.chain_stride * sizeof(double);
  if (r.lds > lds_limit(lanes)) return refuse(kLdsRefusal);
  long long blocks = (chains + ng - 1) / ng;
  if (blocks > 0x7fffffffLL || chains > 0x7fffffffLL) return refuse("too many chains for one launch");
  r.block = kWave;
  if (o.queue && !p.strict && rows > 0 && o.pass == 0 && persistent_by_size(lanes, chains, cus)) {
    blocks = persist_waves_for(cus, blocks);
    r.kind = ABN_KERNEL_PERSISTENT;
    r.key = {kFamRefill, lanes, rows, false, false, false};
    // The quantum grows with the queue's depth (chains per lane group of the launch): a deep queue keeps the GPU full whatever
    // the slicing, every park costs a wavefront ≈ 10 µs of dependent memory traffic, and the tail goes to the speculative
    // kernel anyway; a shallow one needs short slices to start everybody early.  scripts/quantum_sweep.sh, profiles/r04_quantum_sweep.txt:
    // C3 (1.2 chains per group) is best at 256, the C4 shard (2.0) at 256-384, the metaprofile shape (2.4) at 384-768, C4's
    // 200 000 chains (16) at >= 1024.  Results do not depend on it (the persistent kernel is schedule-independent).
    if (o.parking && kQuantum > 0) {
      const long long q = (5LL * kQuantum * chains / (blocks * ng) / 8 + 63) & ~63LL;
      r.quantum = (int)std::min<long long>(4LL * kQuantum, std::max<long long>(kQuantum, q));
      r.tail_cap = tail_cap_for(p, blocks, cus);
    }
  } else {
    r.kind = o.pass != 0 ? ABN_KERNEL_TWO_PASS : rows <= 0 ? ABN_KERNEL_STREAM : ABN_KERNEL_RESIDENT;
    r.key = {kFamFit, lanes, rows, o.pass != 0, p.strict != 0, false};
  }
  r.grid = (unsigned)blocks;
  return r;
}

// ------------------------------------------------------------------------------------------------
// plan level: early bootstraps (abn_plan_run)
// ------------------------------------------------------------------------------------------------
// Phase B needs the BEST start, not the slowest: on a one-window plan whose starts run on the speculative kernel in one
// launch, all resident at once, and whose bootstraps run on the time-sliced persistent kernel, abn_plan_run launches phase B
// once `quorum` of the S starts have finished, lets the stragglers finish beside it and redoes phase B only when one of
// them turns out best.  Never under strict order, with window groups or with fewer than five starts.
struct EarlyRoute {
  bool eligible;
  int quorum;  // starts that must have finished before phase B is launched: S - max(1, S / 5)
};
inline EarlyRoute route_early_bootstraps(const PedigreeRoute& p, int n_windows, int n_starts, int n_boot, int cus,
                                         int window_groups, bool two_pass, bool parking) {
  EarlyRoute e{false, 0};
  if (n_windows != 1 || n_starts < 5 || n_boot <= 0 || p.strict || window_groups > 1) return e;
  const PhaseRoute pa = route_phase(p, 0, n_starts, cus, 0, true, two_pass);
  if (!pa.spec || n_starts > (pick_rmax(p.n, kWave) <= 2 ? 4LL : 3LL) * cus) return e;
  const PhaseRoute pb = route_phase(p, 1, n_boot, cus, 1, true, two_pass);
  LaunchOffer offer;
  offer.queue = true;
  offer.parking = parking;
  const LaunchRoute lb = route_launch(p, pb, n_boot, cus, offer);
  if (lb.status != ABN_OK || lb.kind != ABN_KERNEL_PERSISTENT) return e;
  e.eligible = true;
  e.quorum = n_starts - std::max(1, n_starts / 5);
  return e;
}

}  // namespace abn
