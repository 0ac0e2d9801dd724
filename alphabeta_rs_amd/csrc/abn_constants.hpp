// Sizes the kernels and the host's launch policy (abn_route.hpp) both need: plain constants, no device code, no HIP
// header — the routing compiles into the CPU test shim (host/host_capi.cpp) as it is.
#pragma once

namespace abn {

constexpr int kWave = 64;
constexpr int kPw = 10;  // doubles per entry of the power table in LDS: 9 elements + 1 so that entries are 16-byte aligned
static_assert(kPw % 2 == 0 && kPw >= 9, "load_matrix reads 16-byte aligned pairs");
constexpr int kStreamVec = 4;  // consecutive rows per lane and block in stream mode
#ifndef ABN_STREAM_BLOCKS
#define ABN_STREAM_BLOCKS 6
#endif
constexpr int kStreamBlocks = ABN_STREAM_BLOCKS;  // row blocks a lane keeps in flight per loop iteration
// abn_sweep_kernel (abn_fit_sweep.hpp) holds one wavefront per SIMD where the per-evaluation stream kernel holds two (its
// LDS footprint is about twice as large), so its deep loop keeps twice the row blocks of a lane in flight: the bytes in
// flight per CU stay what they are.  One trip covers kSweepBlocks x kStreamVec x 64 rows; shorter rows take its pair loop.
constexpr int kSweepBlocks = 2 * kStreamBlocks;
constexpr int kStrictRowsPerLane = 8;  // rows per lane and chunk of the strict stream variant (abn_fit_kernel.hpp)

constexpr int kParkHead = 0, kParkTail = 64, kParkAvail = 128, kParkHeaderInts = 192;  // one cache line each
constexpr int kParkShards = 64;  // independent FIFOs (workgroup b uses b mod 64): a cache line serves ~100 M atomics/s

// ------------------------------------------------------------------------------------------------
// records the host and the three fit kernels exchange through memory (each laid out here once)
// ------------------------------------------------------------------------------------------------
// The parked Nelder-Mead state of one chain (FitArgs::state, kStateDoubles doubles per chain), written at an iteration
// boundary by abn_fit_kernel (first pass of a two-pass phase A) or abn_fit_refill_kernel (time slicing, tail hand-over)
// and read by abn_fit_kernel (second pass), abn_fit_refill_kernel or abn_fit_spec_kernel (the tail's resume launch):
constexpr int kStateSimplex = 0;     // [5][4] the vertices in rank order: dimension d of vertex k at 4 k + d
constexpr int kStateCosts = 20;      // [5] their costs
constexpr int kStateBest = 25;       // [4] the best point so far
constexpr int kStateBestCost = 29;   // its cost
constexpr int kStateIterEvals = 30;  // one 64-bit word: iter in the low half, evals in the high half
constexpr int kStateHaveBest = 31;   // one 64-bit word: 0 / 1
constexpr int kStateDoubles = 32;
// Words 30 and 31 have ONE encoding.  abn_fit_refill_kernel and abn_fit_spec_kernel move each as a `long long` behind
// the bits of a double (iter | evals << 32; have_best); abn_fit_kernel sees the two words as four ints at
// (int*)(state + kStateIterEvals) — on the little-endian gfx950 the same bytes:
constexpr int kStateIntIter = 0, kStateIntEvals = 1, kStateIntHaveBest = 2, kStateIntZero = 3;  // [3]: high half of word 31
static_assert(kStateSimplex == 0 && kStateCosts == kStateSimplex + 5 * 4 && kStateBest == kStateCosts + 5 &&
                  kStateBestCost == kStateBest + 4 && kStateIterEvals == kStateBestCost + 1 &&
                  kStateHaveBest == kStateIterEvals + 1 && kStateDoubles == kStateHaveBest + 1,
              "the regions of the parked state tile 0 .. kStateDoubles - 1 exactly");
static_assert(2 * (kStateDoubles - kStateIterEvals) == kStateIntZero + 1, "the int view covers words 30 and 31");

// Status words of a persistent launch (FitArgs::slice_status; the plan holds kSliceWords per phase, abn_plan.hip's
// verify_persistent reads them at the next synchronisation):
constexpr int kSliceError = 0;      // |= kSliceErrLostEntry (abn_common.hpp): a claimed FIFO entry never appeared
constexpr int kSliceFinished = 1;   // += fits finished (results written), the tail's resume launch included
constexpr int kSliceHanded = 2;     // += chains handed to the tail
constexpr int kSliceTailFill = 3;   // the tail list's fill count (FitArgs::susp_count of a launch with tail_cap > 0)
constexpr int kSliceWords = 4;
// ... and the plan's pair of 64-bit words per phase (abn_plan::skipped):
constexpr int kPhaseSkipped = 0;    // evaluations not executed (FitArgs::skipped, the fixed-point skip)
constexpr int kPhaseQueue = 1;      // its low 32 bits: the chain queue of the persistent kernel (FitArgs::queue)
constexpr int kPhaseWords = 2;
// Early bootstraps (abn_plan_run on a quorum of starts, abn_plan.hip): the plan's slots of those words are phase A, phase B
// (the early launch) and the guarded redo of phase B, and behind them, zeroed by the same clear, kEarlyWords 32-bit words:
constexpr int kPhaseSlots = 3, kSlotRedo = 2;
constexpr int kEarlyCount = 0;      // += starts finished in pass 1 of phase A (FitArgs::quorum_words: count, then flag)
constexpr int kEarlyFlag = 1;       // != 0: a quorum of them has: the running starts park at their next iteration boundary
constexpr int kEarlyParked = 2;     // the length of the list of parked starts
constexpr int kEarlyMiss = 3;       // != 0: the selection over all starts chose another start than the early one
constexpr int kEarlySink = 4;       // kSliceWords words the stragglers' resume launch counts into (nobody reads them)
constexpr int kEarlyWords = kEarlySink + kSliceWords;
static_assert(kEarlyFlag == kEarlyCount + 1, "FitArgs::quorum_words: the flag follows the counter");

// FitArgs::gap_tol = kGapTolFactor x abn_options.sd_tolerance.  The factor is what the convergence shortcut rests on: a
// cost gap above it can never test as converged (the proof is in begin_iteration, abn_fit_kernel.hpp).
constexpr double kGapTolFactor = 64.0;

constexpr int kTreeCanon = 0x10040;      // the oracle's `lanes` code: 64 accumulators | mirror-descending steps

constexpr int kSelChunk = 512;  // terms per chunk of the selection kernels' serial sums (abn_aux_kernels.hpp)

// the speculative kernel's exchange area (abn_fit_spec.hpp)
constexpr int kSpecOutcomes = 10;                                   // r@0..3, e@0, c@0..4
constexpr int kSpecTabDoubles = kSpecOutcomes * 12;                 // [outcome][candidate r/e/c][dimension]
constexpr int kSpecPreDoubles = kSpecOutcomes * 3 * 12;             // [outcome][candidate][G (9), penalty, 0.0, pad]
constexpr int kSpecCommDoubles = 8 + 2 * kSpecTabDoubles + 16 + 2 * kSpecPreDoubles + 16;  // cost exchange, two candidate
                                                 // tables, shrink points, two tables of prepared inputs, two control blocks

}  // namespace abn
