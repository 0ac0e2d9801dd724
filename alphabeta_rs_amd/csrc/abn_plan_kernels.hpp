// The kernels only the device-resident plan launches (abn_plan.hip includes this, and nothing else does): the
// materialised bootstrap observations of the stream mode, and the two small kernels of the early bootstraps.
#pragma once
#include "abn_common.hpp"

namespace abn {

// Early bootstraps (abn_plan_run): the selection ran twice through the two selection kernels (abn_aux_kernels.hpp) — over
// the starts finished at the quorum (into the plan's buffers, which phase B reads) and, beside phase B, over all of them
// (into scratch buffers).
// `miss` is raised when the two chose different starts: the early phase B then stops and is redone.
__global__ __launch_bounds__(kWave) void abn_early_compare_kernel(const int32_t* early, const int32_t* all, int W, unsigned* miss) {
  for (int w = threadIdx.x; w < W; w += kWave)
    if (early[w] != all[w]) __hip_atomic_store(miss, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ... and the selection over all starts becomes the plan's (the same bytes when the two agree)
__global__ __launch_bounds__(256) void abn_early_adopt_kernel(const SelectArgs from, const SelectArgs to) {
  const long long rows = (long long)to.W * to.N, n = rows > 4LL * to.W ? rows : 4LL * to.W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    if (i < rows) {
      to.pred[i] = from.pred[i];
      to.resid[i] = from.resid[i];
    }
    if (i < 4LL * to.W) to.model[i] = from.model[i];
    if (i < to.W) to.best_start[i] = from.best_start[i];
  }
}

// ------------------------------------------------------------------------------------------------
// Residual bootstrap observations, materialised once per fit for the stream mode (src/boot_model.rs:50-57):
// dstar[(w*B + b)*N + i] = pred[w*N + i] + resid[w*N + idx[(w*B + b)*N + i]].  The index buffer is read
// once, coalesced; the evaluations then stream dstar (8 B per row) instead of re-gathering through the index
// row (4 B per row + an 8-byte random gather that, for tables beyond LDS, is bound by L2->L1 sector traffic).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void abn_make_dstar_kernel(double* dstar, const double* pred, const double* resid,
                                                             const uint32_t* idx, int N, long long rows_per_window,
                                                             long long total) {
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total;
       t += (long long)gridDim.x * blockDim.x) {
    const long long w = t / rows_per_window;
    const int i = (int)(t % N);
    const size_t wN = (size_t)w * (size_t)N;
    dstar[t] = pred[wN + i] + resid[wN + idx[t]];
  }
}

}  // namespace abn
