// Stand-alone check of alphabeta_rs_amd/csrc/abn_prepare.hpp (host code only, its own main; tests/test_step_prepare_cpu.py
// builds it plain and under -fsanitize=address,undefined and runs it directly).
//
// For a sweep of (chains, slice_cap, eligible or not, two-pass or not, sweep counters or not) the description of what a
// step's preparation clears is applied to heap blocks of exactly each buffer's length and set against a serial model of the
// memsets it replaces, written out below from the launch chain as it was: the words' clear, then per persistent launch
// the status words, the FIFO entries (0xff) and the FIFO headers — for the early phase B, and for the guarded redo in its
// own region.  Checked: the bytes after both are the same (the description covers exactly the union of the memsets'
// ranges, each with its fill byte), no byte is written twice, no range leaves its buffer, every range is a multiple of 4.
//
// What a list is said to leave clear (prep_clean: each slot's status words, each FIFO region, the two-pass counter) is set
// against the bytes the list wrote, for every list above: claimed if and only if every byte of that range was written with
// its fill, and never for a range the plan does not have.  A list given more ranges than it holds says so.
//
// argv[1] = "list": print one line per case instead of checking quietly (the Python test reads them).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../alphabeta_rs_amd/csrc/abn_prepare.hpp"

using namespace abn;

namespace {

constexpr unsigned char kUntouched = 0x5a;

struct Buffers {
  size_t bytes[kPrepBuffers] = {};
  std::unique_ptr<unsigned char[]> mem[kPrepBuffers];   // exactly bytes[b] long: a write past the end is the sanitizer's
  std::unique_ptr<unsigned char[]> hits[kPrepBuffers];  // writes per byte
  void alloc() {
    for (int b = 0; b < kPrepBuffers; ++b) {
      mem[b].reset(new unsigned char[bytes[b] ? bytes[b] : 1]);
      hits[b].reset(new unsigned char[bytes[b] ? bytes[b] : 1]);
      std::memset(mem[b].get(), kUntouched, bytes[b]);
      std::memset(hits[b].get(), 0, bytes[b]);
    }
  }
  void set(int b, size_t off, int fill, size_t n) {   // one memset of the model, or one range of the description
    std::memset(mem[b].get() + off, fill, n);
    for (size_t i = 0; i < n; ++i)
      if (hits[b][off + i] < 255) ++hits[b][off + i];
  }
};

struct Case {
  size_t chains;       // W x max(S, B): sizes the list behind which the two-pass counter lies
  unsigned slice_cap;  // 0: no FIFO
  bool eligible, early, two_pass, sweep;
};

Buffers sized(const Case& k) {
  Buffers b;
  b.bytes[kPrepWords] = kPlanWords64 * 8;
  b.bytes[kPrepFifo] = k.slice_cap ? fifo_bytes(k.slice_cap, k.eligible) : 0;
  b.bytes[kPrepSweep] = k.sweep ? 16 : 0;
  b.bytes[kPrepTail] = k.two_pass ? (k.chains + 1) * 4 : 0;
  b.alloc();
  return b;
}

int failures = 0;
void fail(const Case& k, const char* what, int buffer, size_t at) {
  if (++failures <= 20)
    std::printf("FAIL chains %zu cap %u eligible %d early %d two_pass %d sweep %d: %s (buffer %d, byte %zu)\n", k.chains,
                k.slice_cap, (int)k.eligible, (int)k.early, (int)k.two_pass, (int)k.sweep, what, buffer, at);
}

// the description, applied; returns false when a range is malformed (and does not write it)
bool apply(const Case& k, const PrepList& l, Buffers& b) {
  bool ok = true;
  if (l.n <= 0 || l.n > kPrepMaxRanges) {
    fail(k, "range count", -1, (size_t)l.n);
    return false;
  }
  for (int i = 0; i < l.n; ++i) {
    const PrepRange& r = l.r[i];
    if (r.buffer < 0 || r.buffer >= kPrepBuffers || r.bytes == 0 || r.bytes % 4 || r.offset % 4 ||
        r.offset + r.bytes > b.bytes[r.buffer]) {
      fail(k, "range outside its buffer or not in words", r.buffer, r.offset);
      ok = false;
      continue;
    }
    if (r.fill != 0x00 && r.fill != 0xff) fail(k, "fill byte", r.buffer, r.offset);
    b.set(r.buffer, r.offset, r.fill, r.bytes);
  }
  return ok;
}

void compare(const Case& k, const Buffers& model, const Buffers& got, bool model_may_repeat) {
  for (int b = 0; b < kPrepBuffers; ++b)
    for (size_t i = 0; i < model.bytes[b]; ++i) {
      if (model.mem[b][i] != got.mem[b][i]) return fail(k, model.hits[b][i] ? "byte the memsets cleared is not" : "byte cleared that no memset touched", b, i);
      if (got.hits[b][i] > 1) return fail(k, "ranges overlap", b, i);
      if (!model_may_repeat && model.hits[b][i] > 1) return fail(k, "model overlaps", b, i);
    }
}

// every byte of [off, off + n) exists in buffer `buf` and was written, with `fill`
bool written(const Buffers& b, int buf, size_t off, size_t n, unsigned char fill) {
  if (n == 0 || off + n > b.bytes[buf]) return false;
  for (size_t i = off; i < off + n; ++i)
    if (b.hits[buf][i] == 0 || b.mem[buf][i] != fill) return false;
  return true;
}

// prep_clean of a list against the bytes that list wrote into g (the ranges written out here, not taken from the header)
int clean_lists = 0, clean_claims = 0;
void check_clean(const Case& k, const PrepList& l, const Buffers& g) {
  const PrepClean c = prep_clean(l, k.slice_cap, k.chains);
  const size_t status0 = (size_t)kPhaseSlots * kPhaseWords * 8 + (size_t)kEarlyWords * 4;
  for (int slot = 0; slot < kPhaseSlots; ++slot) {
    const size_t at = status0 + (size_t)kSliceWords * 4 * slot;
    const bool is = written(g, kPrepWords, at, (size_t)kSliceWords * 4, 0x00);
    if (c.status[slot] != is) fail(k, is ? "cleared status words not claimed" : "status words claimed clear that are not", kPrepWords, at);
    clean_claims += c.status[slot];
  }
  const size_t header = (size_t)kParkShards * kParkHeaderInts * 4, entries = (size_t)kParkShards * k.slice_cap * 4;
  for (int region = 0; region < (int)(sizeof c.fifo / sizeof c.fifo[0]); ++region) {
    const size_t base = (size_t)region * (header + entries);
    const bool has = k.slice_cap > 0 && region < (k.eligible ? 2 : 1);
    const bool is = has && written(g, kPrepFifo, base, header, 0x00) && written(g, kPrepFifo, base + header, entries, 0xff);
    if (c.fifo[region] != is) fail(k, is ? "cleared FIFO not claimed" : "FIFO claimed clear that is not (or that the plan lacks)", kPrepFifo, base);
    clean_claims += c.fifo[region];
  }
  const bool is = k.two_pass && written(g, kPrepTail, k.chains * 4, 4, 0x00);
  if (c.two_pass != is) fail(k, is ? "cleared two-pass counter not claimed" : "two-pass counter claimed clear that is not", kPrepTail, k.chains * 4);
  clean_claims += c.two_pass;
  if (l.overflow) fail(k, "list overflowed", -1, (size_t)l.n);
  ++clean_lists;
}

// a list says when a range did not fit, and then claims nothing clear
bool check_overflow() {
  PrepList l;
  for (int i = 0; i < kPrepMaxRanges; ++i) l.add(kPrepWords, plan_status_offset(0) + 4 * (size_t)i, 4, 0x00);
  l.add(kPrepWords, 0, 0, 0x00);   // an empty range takes no place
  if (l.overflow || l.n != kPrepMaxRanges) return false;
  PrepList full;
  full.add(kPrepWords, 0, kPlanWords64 * 8, 0x00);
  if (!prep_clean(full, 0, 0).status[0]) return false;
  for (int i = 1; i <= kPrepMaxRanges; ++i) full.add(kPrepSweep, 0, 8, 0x00);
  l.add(kPrepSweep, 0, 8, 0x00);
  const PrepClean c = prep_clean(full, 0, 0);
  return l.overflow && l.n == kPrepMaxRanges && full.overflow && !c.status[0] && !c.status[1] && !c.status[kSlotRedo];
}

// serial model: the memsets of one persistent launch (launch_fit as it was)
void model_launch(Buffers& m, int slot, unsigned cap, int region, bool status, bool fifo) {
  const size_t early = (size_t)kPhaseSlots * kPhaseWords * 8;
  if (status) m.set(kPrepWords, early + ((size_t)kEarlyWords + (size_t)kSliceWords * slot) * 4, 0x00, (size_t)kSliceWords * 4);
  if (fifo) {
    const size_t region_bytes = (size_t)kParkShards * ((size_t)kParkHeaderInts + cap) * 4, base = (size_t)region * region_bytes;
    m.set(kPrepFifo, base + (size_t)kParkShards * kParkHeaderInts * 4, 0xff, (size_t)kParkShards * cap * 4);   // entries
    m.set(kPrepFifo, base, 0x00, (size_t)kParkShards * kParkHeaderInts * 4);                                  // headers
  }
}

// the whole step (abn_plan_run): words, sweep counters, two-pass counter, phase B's launch, and early: the redo's
void check_step(const Case& k) {
  Buffers m = sized(k), g = sized(k);
  m.set(kPrepWords, 0, 0x00, kPlanWords64 * 8);
  if (k.sweep) {
    m.set(kPrepSweep, 0, 0x00, 8);
    m.set(kPrepSweep, 8, 0x00, 8);
  }
  if (k.two_pass) m.set(kPrepTail, k.chains * 4, 0x00, 4);
  model_launch(m, 1, k.slice_cap, 0, true, k.slice_cap > 0);
  if (k.early) model_launch(m, kSlotRedo, k.slice_cap, 1, true, k.slice_cap > 0);
  const PrepList l = prep_step(k.slice_cap, k.early, k.sweep, k.two_pass, k.chains);
  apply(k, l, g);
  check_clean(k, l, g);
  compare(k, m, g, true);   // the status words' memsets repeat the words' clear: that is what the step drops
}

// one phase on its own (abn_plan_run_phase): the phase's two words, its sweep counter, its launch's three memsets
void check_phase(const Case& k, int phase) {
  Buffers m = sized(k), g = sized(k);
  m.set(kPrepWords, (size_t)kPhaseWords * phase * 8, 0x00, (size_t)kPhaseWords * 8);
  if (k.sweep) m.set(kPrepSweep, (size_t)phase * 8, 0x00, 8);
  if (k.two_pass && phase == 0) m.set(kPrepTail, k.chains * 4, 0x00, 4);
  model_launch(m, phase, k.slice_cap, 0, true, k.slice_cap > 0);
  const PrepList l = prep_phase(phase, k.slice_cap, k.sweep, k.two_pass, k.chains);
  apply(k, l, g);
  check_clean(k, l, g);
  compare(k, m, g, false);
}

// a single launch's own clears, each combination, each slot in its region
void check_launch(const Case& k) {
  for (int slot = 0; slot < kPhaseSlots; ++slot)
    for (int what = 1; what < 4; ++what) {
      const bool status = what & 1, fifo = (what & 2) && k.slice_cap > 0;
      if (!status && !fifo) continue;
      const int region = fifo_region_of(slot, k.eligible);
      if (region >= fifo_regions(k.eligible)) fail(k, "region beyond the plan's", kPrepFifo, (size_t)region);
      Buffers m = sized(k), g = sized(k);
      model_launch(m, slot, k.slice_cap, region, status, fifo);
      const PrepList l = prep_launch(slot, status, fifo, k.slice_cap, region);
      apply(k, l, g);
      check_clean(k, l, g);
      compare(k, m, g, false);
    }
}

}  // namespace

int main(int argc, char** argv) {
  const bool list = argc > 1 && std::strcmp(argv[1], "list") == 0;
  // (chains, capacity): no FIFO; the plan's own rule (abn_plan_create: 16 entries per chain over the shards, and 4096) at
  // the smallest and at the benchmark's plan; odd capacities the rule never yields — the arithmetic must hold for any
  const auto rule = [](size_t chains) { return (unsigned)(chains * 16 / kParkShards + 4096); };
  const struct {
    size_t chains;
    unsigned cap;
  } shapes[] = {{1, 0}, {10000, 0}, {10, rule(10)}, {10000, rule(10000)}, {4097, 65}, {25000, 3}, {7, 1}, {7, 63}};
  int cases = 0;
  for (const auto& sh : shapes)
    for (int eligible = 0; eligible < (sh.cap ? 2 : 1); ++eligible)   // eligibility needs the persistent kernel's buffers
      for (int early = 0; early <= eligible; ++early)                 // an early run needs an eligible plan
        for (int two_pass = 0; two_pass < 2; ++two_pass)
          for (int sweep = 0; sweep < 2; ++sweep) {
            const Case k{sh.chains, sh.cap, eligible != 0, early != 0, two_pass != 0, sweep != 0};
            const int before = failures;
            check_step(k);
            check_phase(k, 0);
            check_phase(k, 1);
            if (!two_pass && !sweep && !early) check_launch(k);   // a launch's own clears know neither
            ++cases;
            if (list)
              std::printf("case chains %zu cap %u eligible %d early %d two_pass %d sweep %d fifo_bytes %zu: %s\n", sh.chains, sh.cap,
                          eligible, early, two_pass, sweep, sh.cap ? fifo_bytes(sh.cap, eligible != 0) : (size_t)0,
                          failures == before ? "ok" : "FAILED");
          }
  // the second region is one region's length behind the first, and the allocation grows by exactly that
  for (unsigned cap : {4096u, 6596u})
    if (fifo_bytes(cap, true) - fifo_bytes(cap, false) != fifo_region_ints(cap) * 4 ||
        fifo_header_offset(cap, 1) != fifo_bytes(cap, false) || fifo_entries_offset(cap, 0) != (size_t)kParkShards * kParkHeaderInts * 4) {
      std::printf("FAIL region arithmetic at cap %u\n", cap);
      ++failures;
    }
  const bool overflow_ok = check_overflow();
  if (!overflow_ok) {
    std::printf("FAIL a list given more than %d ranges does not report it\n", kPrepMaxRanges);
    ++failures;
  }
  if (list) std::printf("clean record: %d lists checked, %d ranges claimed clear\noverflow of %d ranges reported: %s\n", clean_lists,
                        clean_claims, kPrepMaxRanges + 1, overflow_ok ? "ok" : "FAILED");
  if (failures) {
    std::printf("step prepare: %d failure(s) in %d cases\n", failures, cases);
    return 1;
  }
  std::printf("step prepare ok: %d cases\n", cases);
  return 0;
}
