// What a plan's step clears before its fit launches, described once for the host and the device: plain constants and
// host arithmetic in the manner of abn_constants.hpp, no device code, no HIP header (tests/native/step_prepare_main.cpp
// compiles it alone).  abn_step_prepare_kernel (abn_aux_kernels.hpp) fills a list of these ranges in ONE launch; the
// memset form of the same list (one hipMemsetAsync per range, abn_api.hip: clear_ranges) serves outside a step.
// The ranges a persistent launch depends on are named once (status_range, fifo_*_range, two_pass_range): the lists add
// them, and prep_clean reads off a list which of them it leaves clear (PrepClean, kept in abn_plan::clean).
//
// Buffers (PrepBuffer) and what lies in them:
//   kPrepWords  abn_plan::skipped — kPhaseSlots x kPhaseWords 64-bit words (skip counter, chain queue), then kEarlyWords
//               32-bit words of the early bootstraps, then kPhaseSlots x kSliceWords status words: kPlanWords64 x 8 bytes
//   kPrepFifo   abn_plan::slice_buf — fifo_regions() regions of [kParkShards x kParkHeaderInts header ints, fill 0x00]
//               [kParkShards x slice_cap entries, fill 0xff]; region 0 serves phase A and phase B, region 1 (plans eligible
//               for early bootstraps only) the guarded redo of phase B, which is cleared before the early phase B starts
//               using region 0 and so cannot share it
//   kPrepSweep  abn_plan::sweep_passes — one 64-bit pass counter per phase (allocated once the stream sweep was switched on)
//   kPrepTail   abn_plan::susp_list — the int counter behind the W x S entries of a two-pass phase A's list
#pragma once
#include <cstddef>

#include "abn_constants.hpp"

namespace abn {

// The plan's small words, one allocation so that one clear zeroes a step's and one copy fetches them (in 32-bit words
// behind the kPhaseSlots x kPhaseWords 64-bit ones): [kEarlyWords early bootstraps][kPhaseSlots x kSliceWords status]
constexpr size_t kPlanWords64 = (size_t)kPhaseSlots * kPhaseWords + ((size_t)kEarlyWords + (size_t)kPhaseSlots * kSliceWords + 1) / 2;
constexpr size_t kPlanEarlyOffset = (size_t)kPhaseSlots * kPhaseWords * 8;                 // bytes: the early bootstraps' words
constexpr size_t plan_status_offset(int slot) { return kPlanEarlyOffset + ((size_t)kEarlyWords + (size_t)kSliceWords * slot) * 4; }

enum PrepBuffer { kPrepWords = 0, kPrepFifo, kPrepSweep, kPrepTail, kPrepBuffers };

// FIFO regions of a plan and the one a slot's launch parks in
constexpr int fifo_regions(bool early_eligible) { return early_eligible ? 2 : 1; }
constexpr int fifo_region_of(int slot, bool early_eligible) { return early_eligible && slot == kSlotRedo ? 1 : 0; }
constexpr size_t fifo_region_ints(unsigned slice_cap) { return (size_t)kParkShards * ((size_t)kParkHeaderInts + slice_cap); }
constexpr size_t fifo_header_offset(unsigned slice_cap, int region) { return (size_t)region * fifo_region_ints(slice_cap) * 4; }  // bytes
constexpr size_t fifo_entries_offset(unsigned slice_cap, int region) {
  return fifo_header_offset(slice_cap, region) + (size_t)kParkShards * kParkHeaderInts * 4;
}
constexpr size_t fifo_bytes(unsigned slice_cap, bool early_eligible) { return fifo_regions(early_eligible) * fifo_region_ints(slice_cap) * 4; }

struct PrepRange {
  int buffer;            // PrepBuffer
  size_t offset, bytes;  // within it; both multiples of 4
  unsigned char fill;
};

// The ranges a launch depends on, named once: the lists below add them, prep_clean looks for them
// the status words of one slot's persistent launch
constexpr PrepRange status_range(int slot) { return {kPrepWords, plan_status_offset(slot), (size_t)kSliceWords * 4, 0x00}; }
// an empty FIFO: head = tail = available = 0, every entry -1
constexpr PrepRange fifo_header_range(unsigned slice_cap, int region) {
  return {kPrepFifo, fifo_header_offset(slice_cap, region), (size_t)kParkShards * kParkHeaderInts * 4, 0x00};
}
constexpr PrepRange fifo_entries_range(unsigned slice_cap, int region) {
  return {kPrepFifo, fifo_entries_offset(slice_cap, region), (size_t)kParkShards * slice_cap * 4, 0xff};
}
// the counter of a two-pass phase A's list of parked starts (behind its W x S entries)
constexpr PrepRange two_pass_range(size_t list_entries) { return {kPrepTail, list_entries * 4, 4, 0x00}; }

constexpr int kPrepMaxRanges = 8;
struct PrepList {
  int n = 0;
  bool overflow = false;  // a range did not fit: the list is incomplete, clear_ranges refuses it and prep_clean claims nothing
  PrepRange r[kPrepMaxRanges] = {};
  void add(const PrepRange& x) {
    if (x.bytes == 0) return;
    if (n < kPrepMaxRanges) r[n++] = x;
    else overflow = true;
  }
  void add(int buffer, size_t offset, size_t bytes, unsigned char fill) { add(PrepRange{buffer, offset, bytes, fill}); }
  // every byte of x is written by the list, with x's fill (an empty x: no such range in this plan, never covered)
  bool covers(const PrepRange& x) const {
    if (x.bytes == 0 || overflow) return false;
    size_t at = x.offset;
    const size_t end = x.offset + x.bytes;
    for (int k = 0; k < n && at < end; ++k)   // each pass extends the covered prefix or ends the search
      for (int i = 0; i < n; ++i)
        if (r[i].buffer == x.buffer && r[i].fill == x.fill && r[i].offset <= at && at < r[i].offset + r[i].bytes) {
          at = r[i].offset + r[i].bytes;
          break;
        }
    return at >= end;
  }
};

inline void prep_fifo(PrepList& l, unsigned slice_cap, int region) {
  l.add(fifo_header_range(slice_cap, region));
  l.add(fifo_entries_range(slice_cap, region));
}
inline void prep_status(PrepList& l, int slot) { l.add(status_range(slot)); }
// skip counter and chain queue of one phase (abn_plan_run_phase), with the phase's pass counter of the stream sweep
inline void prep_phase_words(PrepList& l, int phase, bool sweep_counters) {
  l.add(kPrepWords, (size_t)kPhaseWords * phase * 8, (size_t)kPhaseWords * 8, 0x00);
  if (sweep_counters) l.add(kPrepSweep, (size_t)phase * 8, 8, 0x00);
}
inline void prep_two_pass(PrepList& l, size_t list_entries) { l.add(two_pass_range(list_entries)); }

// What a run of ONE phase through abn_plan_run_phase clears at its head: the phase's words and everything its launch may
// use (a launch that turns out not to be persistent leaves the status words and the FIFO unused)
inline PrepList prep_phase(int phase, unsigned slice_cap, bool sweep_counters, bool two_pass, size_t list_entries) {
  PrepList l;
  prep_phase_words(l, phase, sweep_counters);
  prep_status(l, phase);
  if (slice_cap > 0) prep_fifo(l, slice_cap, 0);
  if (two_pass && phase == 0) prep_two_pass(l, list_entries);
  return l;
}

// What abn_plan_run clears at the head of a step: all of the plan's words (every slot's status words, the early
// bootstraps' counters and flags), both pass counters, the FIFO of region 0 and — early: the step is an early-bootstraps
// run — that of the redo's region.  A stopped early phase B leaves region 0 dirty and a redo that ran region 1: the next
// step's head covers both.  A step whose phase A parks in region 0 (time slicing) leaves it dirty for phase B, which then
// clears it again with a launch of its own (prep_launch).
inline PrepList prep_step(unsigned slice_cap, bool early, bool sweep_counters, bool two_pass, size_t list_entries) {
  PrepList l;
  l.add(kPrepWords, 0, kPlanWords64 * 8, 0x00);
  if (sweep_counters) l.add(kPrepSweep, 0, 16, 0x00);
  if (slice_cap > 0) prep_fifo(l, slice_cap, 0);
  if (slice_cap > 0 && early) prep_fifo(l, slice_cap, 1);
  if (two_pass) prep_two_pass(l, list_entries);
  return l;
}

// What a single persistent launch needs where no head covered it: its status words and, when it time-slices, its FIFO
inline PrepList prep_launch(int slot, bool status, bool fifo, unsigned slice_cap, int region) {
  PrepList l;
  if (status) prep_status(l, slot);
  if (fifo) prep_fifo(l, slice_cap, region);
  return l;
}

// What a persistent launch may find clear and use without a clear of its own: the status words per slot, the FIFO per
// region, the two-pass list's counter.  A launch marks what it uses as dirty (abn_api.hip: launch_fit; abn_plan.hip: launch_phase).
constexpr int kFifoRegionsMax = fifo_regions(true);
struct PrepClean {
  bool status[kPhaseSlots] = {};
  bool fifo[kFifoRegionsMax] = {};
  bool two_pass = false;
};

// What a list leaves clear — read off the list itself, so that the record cannot claim what was not written: clear exactly
// when the list covers all of the range with its fill byte.  slice_cap 0: the plan has no FIFO.
inline PrepClean prep_clean(const PrepList& l, unsigned slice_cap, size_t list_entries) {
  PrepClean c;
  for (int slot = 0; slot < kPhaseSlots; ++slot) c.status[slot] = l.covers(status_range(slot));
  for (int region = 0; region < kFifoRegionsMax; ++region)
    c.fifo[region] = l.covers(fifo_header_range(slice_cap, region)) && l.covers(fifo_entries_range(slice_cap, region));
  c.two_pass = l.covers(two_pass_range(list_entries));
  return c;
}

}  // namespace abn
