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
constexpr int kStrictRowsPerLane = 8;  // rows per lane and chunk of the strict stream variant (abn_fit_kernel.hpp)

constexpr int kParkHead = 0, kParkTail = 64, kParkAvail = 128, kParkHeaderInts = 192;  // one cache line each
constexpr int kParkShards = 64;  // independent FIFOs (workgroup b uses b mod 64): a cache line serves ~100 M atomics/s

constexpr int kTreeCanon = 0x10040;      // the oracle's `lanes` code: 64 accumulators | mirror-descending steps

constexpr int kSelChunk = 512;  // terms per chunk of the selection kernels' serial sums (abn_aux_kernels.hpp)

// the speculative kernel's exchange area (abn_fit_spec.hpp)
constexpr int kSpecOutcomes = 10;                                   // r@0..3, e@0, c@0..4
constexpr int kSpecTabDoubles = kSpecOutcomes * 12;                 // [outcome][candidate r/e/c][dimension]
constexpr int kSpecPreDoubles = kSpecOutcomes * 3 * 12;             // [outcome][candidate][G (9), penalty, 0.0, pad]
constexpr int kSpecCommDoubles = 8 + 2 * kSpecTabDoubles + 16 + 2 * kSpecPreDoubles + 16;  // cost exchange, two candidate
                                                 // tables, shrink points, two tables of prepared inputs, two control blocks

}  // namespace abn
