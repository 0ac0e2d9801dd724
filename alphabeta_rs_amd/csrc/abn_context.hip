// The fit path's host-only part of the C-ABI (include/abneutral.h): the pedigree topology, the options, the context's life
// cycle with the status strings, and the host-side Philox generators.  No kernel header is included and no device code
// is emitted here; the kernels and their launchers are abn_api.hip's, the device-resident plan is abn_plan.hip's.
#include "abn_fit_host.hpp"

using namespace abn;

// ------------------------------------------------------------------------------------------------
// pedigree topology: distinct (t0, t1-t0, t2-t0) triples, src/divergence.rs:52,57-58
// ------------------------------------------------------------------------------------------------
static int as_i8(double x) {  // Rust `f64 as i8`: truncate, saturate, NaN -> 0
  if (x != x) return 0;
  if (x >= 127.0) return 127;
  if (x <= -128.0) return -128;
  return (int)x;
}

int abn::build_topology(const double* rows, int n, int stride, Topology& t) {
  if (!rows || n <= 0) return ABN_ERR_INVALID_ARG;
  t.N = n;
  t.tri.clear();
  t.tid.resize((size_t)n);
  std::unordered_map<uint32_t, uint32_t> seen;
  int tmax = 0;
  for (int i = 0; i < n; ++i) {
    const int t0 = as_i8(rows[(size_t)i * stride + 0]);
    const int t1 = as_i8(rows[(size_t)i * stride + 1]);
    const int t2 = as_i8(rows[(size_t)i * stride + 2]);
    // The reference inverts G for negative exponents (src/divergence.rs:17-19) and its i8 subtraction
    // can wrap; neither is meaningful for a pedigree, so such rows are rejected.
    if (t0 < 0 || t1 < t0 || t2 < t0) return ABN_ERR_BAD_PEDIGREE;
    const int ea = t1 - t0, eb = t2 - t0;
    tmax = std::max(tmax, std::max(t0, std::max(ea, eb)));
    const uint32_t key = (uint32_t)t0 | ((uint32_t)ea << 8) | ((uint32_t)eb << 16);
    auto it = seen.find(key);
    uint32_t id;
    if (it == seen.end()) {
      id = (uint32_t)t.tri.size();
      if (id >= 65535u) return ABN_ERR_INVALID_ARG;
      seen.emplace(key, id);
      t.tri.push_back(key);
    } else {
      id = it->second;
    }
    t.tid[(size_t)i] = (uint16_t)id;
  }
  t.K = (int)t.tri.size();
  t.T = tmax;
  t.TP = tmax + 1;
  t.KP = (t.K + 1) & ~1;
  t.chain_stride = scratch_stride(t.TP, t.KP);
  return ABN_OK;
}

int abn::upload_topology(abn_ctx* c, const Topology& t, DevTopology& d) {
  if (int rc = upload(c, d.tri, t.tri.data(), t.tri.size())) return rc;
  if (int rc = upload(c, d.tid, t.tid.data(), t.tid.size())) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ABN_OK;
}

std::vector<double> abn::column3(const double* pedigree, int n) {
  std::vector<double> d((size_t)n);
  for (int i = 0; i < n; ++i) d[(size_t)i] = pedigree[(size_t)i * 4 + 3];
  return d;
}

// ------------------------------------------------------------------------------------------------
// options
// ------------------------------------------------------------------------------------------------
extern "C" void abn_default_options(abn_options* o) {
  if (!o) return;
  o->seed = 20260101ull;
  o->lanes_per_chain = 0;
  o->strict_order = 0;
  o->shrink_on_failed_contraction = 0;
  o->max_iters_start = 10000;  // src/ab_neutral.rs:62
  o->max_iters_boot = 1000;    // src/boot_model.rs:81
  o->stream_mode = 0;
  o->sd_tolerance = 2.220446049250313e-16;  // f64::EPSILON
  o->window_groups = 0;
  o->no_fixed_point_skip = 0;
}

abn_options abn::resolve(const abn_options* o) {
  abn_options d;
  abn_default_options(&d);
  if (o) d = *o;
  return d;
}

// The summation order of a pedigree (abn_options.strict_order: -1 tree, 0 auto, 1 serial) resolved to 0 / 1.  Auto sums
// pedigrees of up to kSerialSumMaxRows rows SERIALLY in row order — the reference's `square_sum += ...`
// (src/structs.rs:206-213), where a serial sum costs nothing measurable and the bundled data/ pedigree (6 rows: the
// north star's parity target, on which `weight` is not identified and a last-ulp difference in a cost can move a
// bootstrap row by O(1)) is then bit-equal to the reference order by DEFAULT.  Like the tree, a function of the pedigree
// (and the options) alone: never of the launch.  An explicit lanes_per_chain keeps its per-lane tree.
abn_options abn::resolve_for(const abn_options* o, int n_rows) {
  abn_options d = resolve(o);
  if (d.strict_order == 0 && d.lanes_per_chain == 0 && n_rows <= kSerialSumMaxRows) d.strict_order = 1;
  else if (d.strict_order < 0) d.strict_order = 0;
  return d;
}

void abn::fill_options(FitArgs& a, const abn_options& o, const PedigreeRoute& pr) {
  a.seed = o.seed;
  a.shrink_variant = o.shrink_on_failed_contraction ? 1 : 0;
  a.no_skip = o.no_fixed_point_skip ? 1 : 0;
  a.sd_tol = o.sd_tolerance;
  a.gap_tol = kGapTolFactor * o.sd_tolerance;
  a.strict = pr.strict;  // = (strict_order of resolve_for) != 0: route_pedigree is given that value
}

// iteration budgets must leave room for the 32-bit evaluation counters (at most 2 evaluations per iteration plus the
// 4 of a shrink); lane counts are 0 (auto) or a power of two up to the wavefront; the tolerance must compare
const char* abn::options_error(const abn_options& o) {
  if (o.max_iters_start < 0 || o.max_iters_start > (1 << 28) || o.max_iters_boot < 0 || o.max_iters_boot > (1 << 28))
    return "max_iters_start / max_iters_boot must be in 0 .. 2^28";
  if (!(o.lanes_per_chain == 0 || o.lanes_per_chain == 8 || o.lanes_per_chain == 16 || o.lanes_per_chain == 32 ||
        o.lanes_per_chain == 64))
    return "lanes_per_chain must be 0 (auto), 8, 16, 32 or 64";
  if (o.sd_tolerance != o.sd_tolerance) return "sd_tolerance is NaN";
  if (o.stream_mode < 0 || o.stream_mode > 1) return "stream_mode must be 0 or 1";
  if (o.window_groups < 0) return "window_groups must be >= 0";
  if (o.strict_order < -1 || o.strict_order > 1) return "strict_order must be -1 (tree), 0 (auto) or 1 (serial)";
  return nullptr;
}

// The residual reduction tree of a pedigree (abn_options.lanes_per_chain; abn_fit_info.lanes): host arithmetic on
// the topology alone — no device, no launch size.
extern "C" int abn_reduction_tree(const abn_options* opts, const double* generations, int32_t n_rows, int32_t* tree) {
  if (!generations || n_rows <= 0 || !tree) return ABN_ERR_INVALID_ARG;
  if (options_error(resolve(opts))) return ABN_ERR_INVALID_ARG;
  const abn_options o = resolve_for(opts, n_rows);
  Topology t;
  const int rc = build_topology(generations, n_rows, 3, t);
  if (rc) return rc;
  *tree = route_pedigree(n_rows, t.K, t.T, o.lanes_per_chain, o.strict_order).reported_tree;
  return ABN_OK;
}

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
extern "C" int abn_version(void) { return ABN_VERSION_MAJOR * 100 + ABN_VERSION_MINOR; }

extern "C" int abn_device_count(int* count) {
  if (!count) return ABN_ERR_INVALID_ARG;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    *count = 0;
    return ABN_ERR_NO_DEVICE;
  }
  *count = n;
  return n > 0 ? ABN_OK : ABN_ERR_NO_DEVICE;
}

extern "C" int abn_init(int device_ordinal, void* stream, abn_ctx** out) {
  if (!out) return ABN_ERR_INVALID_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return ABN_ERR_NO_DEVICE;
  if (device_ordinal < 0 || device_ordinal >= n) return ABN_ERR_INVALID_ARG;
  if (hipSetDevice(device_ordinal) != hipSuccess) return ABN_ERR_HIP;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) return ABN_ERR_HIP;
  // the library holds gfx950 code only, and its one-chain-per-workgroup kernels opt in to a CU's whole 160 KiB of LDS
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0 || prop.multiProcessorCount <= 0 ||
      (size_t)prop.maxSharedMemoryPerMultiProcessor < kMaxDynLds)
    return ABN_ERR_NO_DEVICE;
  abn_ctx* c = new (std::nothrow) abn_ctx();
  if (!c) return ABN_ERR_HIP;
  c->device = device_ordinal;
  c->cus = prop.multiProcessorCount;
  c->lds_per_cu = (size_t)prop.maxSharedMemoryPerMultiProcessor;
  if (stream == ABN_STREAM_DEFAULT) {
    c->stream = nullptr;  // the null stream
    c->own_stream = false;
  } else if (stream) {
    c->stream = (hipStream_t)stream;
    c->own_stream = false;
  } else {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
      delete c;
      return ABN_ERR_HIP;
    }
    c->own_stream = true;
  }
  *out = c;
  return ABN_OK;
}

extern "C" int abn_device_info(const abn_ctx* c, int32_t* out4) {
  if (!c || !out4) return ABN_ERR_INVALID_ARG;
  out4[0] = c->cus;
  out4[1] = (int32_t)(c->lds_per_cu / 1024);
  out4[2] = (int32_t)persist_waves(c->cus);
  out4[3] = (int32_t)persist_waves_small(c->cus);
  return ABN_OK;
}

extern "C" int abn_shutdown(abn_ctx* c) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  for (auto st : c->side) (void)hipStreamDestroy(st);
  (void)hipSetDevice(c->device);
  c->pool->clear();
  c->pool->closed = true;
  delete c;
  return ABN_OK;
}

extern "C" const char* abn_last_error(const abn_ctx* c) { return c ? c->err.c_str() : "null context"; }

extern "C" const char* abn_status_string(int s) {
  switch (s) {
    case ABN_OK: return "ok";
    case ABN_ERR_INVALID_ARG: return "invalid argument";
    case ABN_ERR_BAD_PEDIGREE: return "bad pedigree (generation outside 0..127 or t1/t2 < t0)";
    case ABN_ERR_NO_DEVICE: return "no HIP device";
    case ABN_ERR_HIP: return "HIP runtime error";
    case ABN_ERR_NO_FINITE_FIT: return "no start produced a finite fit";
    case ABN_ERR_STATE: return "plan used out of order";
    default: return "unknown status";
  }
}

// ------------------------------------------------------------------------------------------------
// deterministic inputs (host side)
// ------------------------------------------------------------------------------------------------
// Model::new, src/structs.rs:78-96, five vertices per start (src/ab_neutral.rs:49-55)
extern "C" int abn_gen_start_simplices(uint64_t seed, uint32_t window, int32_t n_starts, double max_divergence,
                                       double* simplex0) {
  if (!simplex0 || n_starts < 0) return ABN_ERR_INVALID_ARG;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  double mx = max_divergence;
  if (!(max_divergence > 0.0)) mx = 0.1;  // :80-83
  for (int32_t s = 0; s < n_starts; ++s)
    for (uint32_t v = 0; v < 5; ++v) {
      uint32_t r0[4], r1[4];
      philox4x32_10(0u, (uint32_t)s * 5u + v, window, kTagStart, k0, k1, r0);
      philox4x32_10(1u, (uint32_t)s * 5u + v, window, kTagStart, k0, k1, r1);
      double* o = simplex0 + ((size_t)s * 5 + v) * 4;
      o[0] = std::pow(10.0, uniform_from(r0[0], r0[1], -9.0, -2.0));
      o[1] = std::pow(10.0, uniform_from(r0[2], r0[3], -9.0, -2.0));
      o[2] = uniform_from(r1[0], r1[1], 0.0, 0.1);
      o[3] = uniform_from(r1[2], r1[3], 0.0, mx);
    }
  return ABN_OK;
}

extern "C" int abn_gen_boot_simplices(uint64_t seed, uint32_t window, uint32_t b0, int64_t nb, const double params[4],
                                      double* simplex0) {
  if (!simplex0 || !params || nb < 0) return ABN_ERR_INVALID_ARG;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int64_t i = 0; i < nb; ++i) {
    double* o = simplex0 + (size_t)i * 20;
    for (int d = 0; d < 4; ++d) o[d] = params[d];
    for (uint32_t v = 1; v < 5; ++v) {
      uint32_t r0[4], r1[4];
      philox4x32_10((v - 1u) * 2u + 0u, b0 + (uint32_t)i, window, kTagJitter, k0, k1, r0);
      philox4x32_10((v - 1u) * 2u + 1u, b0 + (uint32_t)i, window, kTagJitter, k0, k1, r1);
      o[4 * v + 0] = vary_one(params[0], r0[0], r0[1]);
      o[4 * v + 1] = vary_one(params[1], r0[2], r0[3]);
      o[4 * v + 2] = vary_one(params[2], r1[0], r1[1]);
      o[4 * v + 3] = vary_one(params[3], r1[2], r1[3]);
    }
  }
  return ABN_OK;
}
