// The analysis of bootstrap tables, on the host (abn_analyze) and on the device (abn_analyze_batch*, and
// abn::analyze_device_table for abn_plan_analyze).  Kernel: abn_analyze.hpp.
#include "abn_host.hpp"
#include "abn_analyze.hpp"

using namespace abn;

// ------------------------------------------------------------------------------------------------
// src/analysis.rs:50-98 on the host (ndarray mean / Welford std with mul_add, ndarray-stats Linear CI)
// ------------------------------------------------------------------------------------------------
extern "C" int abn_analyze(const double* raw, int64_t n_boot, double* out32) {
  if (!raw || !out32 || n_boot <= 0) return ABN_ERR_INVALID_ARG;
  const size_t B = (size_t)n_boot;
  // the quantiles sort with `<`: a table with a NaN entry or a NaN beta / alpha is refused, out32 untouched (the
  // reference converts to n64, which rejects NaN, :57-58)
  for (size_t i = 0; i < B; ++i)
    if (abn_analyze_row_is_bad(raw + 7 * i)) return ABN_ERR_NO_FINITE_FIT;
  std::vector<double> col(B), sorted(B);
  static const int src_col[8] = {0, 1, -1, 2, 3, 4, 5, 6};
  for (int k = 0; k < 8; ++k) {
    const int cidx = src_col[k];
    for (size_t i = 0; i < B; ++i)
      col[i] = cidx < 0 ? raw[7 * i + 1] / raw[7 * i + 0] : raw[7 * i + (size_t)cidx];  // beta / alpha, :54
    double mean;
    if (cidx < 0) {  // contiguous Array1 -> ndarray's eight-lane unrolled fold
      double part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      size_t i = 0;
      for (; i + 8 <= B; i += 8)
        for (int q = 0; q < 8; ++q) part[q] = part[q] + col[i + (size_t)q];
      double acc = 0.0;
      acc = acc + (part[0] + part[4]);
      acc = acc + (part[1] + part[5]);
      acc = acc + (part[2] + part[6]);
      acc = acc + (part[3] + part[7]);
      for (; i < B; ++i) acc = acc + col[i];
      mean = acc / (double)B;
    } else {  // strided column view -> plain fold
      double acc = 0.0;
      for (size_t i = 0; i < B; ++i) acc = acc + col[i];
      mean = acc / (double)B;
    }
    double wmean = 0.0, sum_sq = 0.0;
    for (size_t i = 0; i < B; ++i) {
      const double delta = col[i] - wmean;
      wmean = wmean + delta / (double)(i + 1);
      sum_sq = std::fma(col[i] - wmean, delta, sum_sq);
    }
    const double sd = std::sqrt(sum_sq / ((double)B - 1.0));
    sorted = col;
    std::sort(sorted.begin(), sorted.end());
    const double qs[2] = {0.025, 0.975};
    double ci[2];
    for (int q = 0; q < 2; ++q) {
      const double fi = qs[q] * (double)(B - 1);
      const size_t lo = (size_t)std::floor(fi), hi = (size_t)std::ceil(fi);
      const double frac = fi - std::trunc(fi);
      ci[q] = sorted[lo] + frac * (sorted[hi] - sorted[lo]);
    }
    out32[k] = mean;
    out32[8 + k] = sd;
    out32[16 + k] = ci[0];
    out32[24 + k] = ci[1];
  }
  return ABN_OK;
}

// ------------------------------------------------------------------------------------------------
// src/analysis.rs:50-98 on the device, every window of a table in one launch (abn_analyze.hpp)
// ------------------------------------------------------------------------------------------------
static int analyze_check(abn_ctx* c, const void* raw, int32_t W, int64_t B, const void* out) {
  if (!raw || !out || W < 0 || B <= 0) return set_err(c, ABN_ERR_INVALID_ARG, "null/size");
  if (B > 0x7fffffffLL) return set_err(c, ABN_ERR_INVALID_ARG, "n_boot above 2^31 - 1");
  return ABN_OK;
}

static int analyze_enqueue(abn_ctx* c, const double* draw, int W, long long B, double* dout, int32_t* dfb) {
  for (int w0 = 0; w0 < W; w0 += kAnMaxWindowsPerLaunch) {
    const int wn = std::min(kAnMaxWindowsPerLaunch, W - w0);
    hipLaunchKernelGGL(abn_analyze_kernel, dim3((unsigned)wn * 8u), dim3(kAnThreads), 0, c->stream,
                       AnalyzeArgs{draw, dout, dfb, B, w0});
    HIPCHK(c, hipGetLastError());
  }
  return ABN_OK;
}

// ABN_ERR_NO_FINITE_FIT once everything has been written, as abn_plan_download
static int analyze_verdict(abn_ctx* c, const int32_t* fb, int W) {
  for (int w = 0; w < W; ++w)
    if (fb[w] >= 0)
      return set_err(c, ABN_ERR_NO_FINITE_FIT, "window " + std::to_string(w) + ": bootstrap " + std::to_string(fb[w]) +
                                                   " has no finite fit: its analysis is NaN");
  return ABN_OK;
}

int abn::analyze_device_table(abn_ctx* c, const double* draw, int32_t W, int64_t B, double* out, int32_t* first_bad) {
  if (int rc = analyze_check(c, draw, W, B, out)) return rc;
  if (W == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<double> dout;
  DevBuf<int32_t> dfb;
  HIPCHK(c, dout.alloc((size_t)W * 32));
  HIPCHK(c, dfb.alloc((size_t)W));
  if (int rc = analyze_enqueue(c, draw, W, B, dout.p, dfb.p)) return rc;
  std::vector<int32_t> fb((size_t)W);
  HIPCHK(c, hipMemcpyAsync(out, dout.p, dout.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(fb.data(), dfb.p, dfb.bytes(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (first_bad) std::copy(fb.begin(), fb.end(), first_bad);
  return analyze_verdict(c, fb.data(), W);
}

extern "C" int abn_analyze_batch_dev(abn_ctx* c, const void* dev_raw, int32_t n_windows, int64_t n_boot, void* dev_out,
                                     void* dev_first_bad, double* kernel_ms) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = analyze_check(c, dev_raw, n_windows, n_boot, dev_out)) return rc;
  if (n_windows == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<int32_t> dfb;  // the verdict needs first_bad whether or not the caller wants it
  if (!dev_first_bad) HIPCHK(c, dfb.alloc((size_t)n_windows));
  int32_t* fbp = dev_first_bad ? (int32_t*)dev_first_bad : dfb.p;
  EventPair ev;
  if (int rc = ev.begin(c, kernel_ms != nullptr)) return rc;
  if (int rc = analyze_enqueue(c, (const double*)dev_raw, n_windows, n_boot, (double*)dev_out, fbp)) return rc;
  if (int rc = ev.end(c, kernel_ms)) return rc;
  std::vector<int32_t> fb((size_t)n_windows);
  HIPCHK(c, hipMemcpyAsync(fb.data(), fbp, fb.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return analyze_verdict(c, fb.data(), n_windows);
}

extern "C" int abn_analyze_batch(abn_ctx* c, const double* raw, int32_t n_windows, int64_t n_boot, double* out,
                                 int32_t* first_bad) {
  if (!c) return ABN_ERR_INVALID_ARG;
  if (int rc = analyze_check(c, raw, n_windows, n_boot, out)) return rc;
  if (n_windows == 0) return ABN_OK;
  HIPCHK(c, hipSetDevice(c->device));
  PoolScope pool_scope(c);
  DevBuf<double> draw;
  HIPCHK(c, draw.alloc((size_t)n_windows * (size_t)n_boot * 7));
  HIPCHK(c, hipMemcpyAsync(draw.p, raw, draw.bytes(), hipMemcpyHostToDevice, c->stream));
  return analyze_device_table(c, draw.p, n_windows, n_boot, out, first_bad);  // synchronises: draw is freed after it
}
