// What the fit path's translation units share on the host — abn_context.hip (topology, options, the context), abn_api.hip
// (the kernel table, the launchers, the one-shot entries) and abn_plan.hip (the device-resident plan and the drop-in
// entries on it).  Declarations, with the templates that must be visible where they are used (the copy helpers upload and
// to_host: abn_host.hpp), and no kernel header: abn_api.hip alone includes abn_device.hpp.  Not part of the C-ABI.
#pragma once
#include "abn_host.hpp"
#include "abn_common.hpp"
#include "abn_route.hpp"
#include "abn_prepare.hpp"

namespace abn {
// ------------------------------------------------------------------------------------------------
// abn_context.hip: the pedigree topology — distinct (t0, t1-t0, t2-t0) triples, src/divergence.rs:52,57-58
// ------------------------------------------------------------------------------------------------
struct Topology {
  int N = 0, K = 0, T = 0, TP = 0, KP = 0, chain_stride = 0;
  std::vector<uint32_t> tri;
  std::vector<uint16_t> tid;
};
struct DevTopology {
  DevBuf<uint32_t> tri;
  DevBuf<uint16_t> tid;
};
// rows: n rows with `stride` doubles each, generations in the first three columns
int build_topology(const double* rows, int n, int stride, Topology& t);
// ... to the device, the stream synchronised
int upload_topology(abn_ctx* c, const Topology& t, DevTopology& d);
// the observed divergences of a four-column pedigree
std::vector<double> column3(const double* pedigree, int n);

// the topology fields every kernel's argument struct starts with
template <class Args>
void fill_topology(Args& a, const Topology& t, const DevTopology& d) {
  a.tri = d.tri.p;
  a.tid = d.tid.p;
  a.N = t.N;
  a.K = t.K;
  a.T = t.T;
  a.TP = t.TP;
}

// ------------------------------------------------------------------------------------------------
// abn_context.hip: options
// ------------------------------------------------------------------------------------------------
// Auto summation order (abn_options.strict_order == 0) sums pedigrees of up to this many rows serially (resolve_for)
constexpr int kSerialSumMaxRows = 16;
// the caller's options, or the defaults for null
abn_options resolve(const abn_options* o);
// ... with strict_order resolved to 0 / 1 for a pedigree of n_rows rows
abn_options resolve_for(const abn_options* o, int n_rows);
// the refusal text of options no entry point takes, or null
const char* options_error(const abn_options& o);
// what every fit launch takes from the resolved options and the pedigree's route
void fill_options(FitArgs& a, const abn_options& o, const PedigreeRoute& pr);

// ------------------------------------------------------------------------------------------------
// abn_api.hip: the launchers
// ------------------------------------------------------------------------------------------------
// The buffers the ranges of abn_prepare.hpp lie in, and their lengths in bytes
struct PrepBases {
  void* base[kPrepBuffers] = {};
  size_t bytes[kPrepBuffers] = {};
};
// What a launch that may be persistent brings along: the buffers its status words and its FIFO lie in (abn_prepare.hpp),
// which slot and region are its own, and the plan's record of what is still clear.  launch_fit clears what is not, in one
// launch, once the route is known, and marks what the launch uses as dirty in that record.
struct LaunchClear {
  PrepBases bases;
  PrepClean* clean = nullptr;
  int slot = 0, region = 0;
};
// the ranges of `l` filled on stream st, in one launch or (one_launch = false) one memset per range
int clear_ranges(abn_ctx* c, const PrepList& l, const PrepBases& b, hipStream_t st, bool one_launch = true);
// a.W x a.C chains as route_launch decides; kind (nullable): the ABN_KERNEL_* code of what was launched
int launch_fit(abn_ctx* c, const PedigreeRoute& pr, const PhaseRoute& ph, FitArgs a, const LaunchOffer& offer, hipStream_t st,
               int* kind = nullptr, LaunchClear* lc = nullptr);
// the chains parked in a's list resume in the speculative kernel and run to their end
int launch_tail_resume(abn_ctx* c, const PedigreeRoute& pr, FitArgs a, int cap, hipStream_t st);
// the two selection kernels: one model per workgroup, then one workgroup per window
int launch_select(abn_ctx* c, const SelectArgs& s, size_t lds, hipStream_t st);
// the bootstrap indices of w windows x b bootstraps x n rows, on the context's stream
int launch_gen_idx(abn_ctx* c, uint32_t* idx, int n, int b, int w, uint64_t seed, uint32_t woff, uint32_t boff,
                   const uint32_t* wid = nullptr);
}  // namespace abn
