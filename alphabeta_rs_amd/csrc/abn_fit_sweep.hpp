// abn_sweep_kernel: the streamed fit with ONE pass over a chain's rows per Nelder-Mead iteration (opt-in:
// abn_plan_set_stream_sweep, abn_fit_batch_sweep; LaunchOffer::sweep in abn_route.hpp).
//
// The stream form of abn_fit_kernel re-reads a chain's rows once per cost evaluation, about 1.75 times per iteration.
// Yet all that NelderMead::next_iter can ask for in an iteration is known at its start: the reflection xr, the expansion
// xe = x0 + 2 (xr - x0) and the contraction xc = x0 + (x4 - x0) / 2.  This kernel builds the three candidates' dt tables
// (each through the one power table, one after the other), streams the rows once and keeps three accumulators per lane.
// Each accumulator adds its own terms in the order of the per-evaluation kernel — block by block, row by row, then the
// xor-butterfly — so every cost is that kernel's bit for bit: the tree code stays 64 | (kStreamVec - 1) << 8.  The decision
// is then taken on the stored costs with the predicates of abn_fit_kernel's loop; a cost the reference would not have
// asked for is neither counted nor looked at.  Solver::init and NelderMead::shrink evaluate one candidate per pass.
//
// One wavefront per chain (G = 64), tree order only, one pass.  RMAX = 0: the deep loop (kSweepBlocks row blocks of a lane
// in flight, for rows of at least one such trip); RMAX = -1: pairs of blocks (mid-size pedigrees).
// LDS per workgroup: kPw (T+1) + 3 KP + 4 doubles (abn_route.hpp: sweep_stride).
#pragma once
#include "abn_common.hpp"

namespace abn {

// One pass over the rows of a streamed chain for NC candidates at once.  Lane l owns the row blocks 4 (l + 64 q) .. + 3,
// q = 0, 1, ...; SNB of them are in flight per trip of the deep loop, then pairs, then single (possibly partial) blocks.
// Each loaded observation and triple id serves NC terms; acc[c] sees the same additions in the same order whatever SNB and
// NC are.
template <int NC, int SNB>
__device__ __forceinline__ void sweep_rows(const FitArgs& a, int lane, const uint32_t* idx_row, size_t wN, size_t dN,
                                           const double* const (&dt)[NC], const double (&ic)[NC], const double (&pen)[NC],
                                           double (&acc)[NC]) {
  constexpr int V = kStreamVec;
  constexpr int stride = V * kWave;
  const int N = a.N;
  int base = V * lane;
  auto blocks = [&](auto nbk) {
    constexpr int NB = decltype(nbk)::value;
    for (; base + (NB - 1) * stride + V <= N; base += NB * stride) {
      double d[NB * V];
      u16x4 tq[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) tq[b] = *reinterpret_cast<const u16x4*>(a.tid + base + b * stride);
      if (a.dmode == 1) {
        u32x4 ix[NB];
        f64x2 pl[NB], ph[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          ix[b] = *reinterpret_cast<const u32x4*>(idx_row + base + b * stride);
          pl[b] = *reinterpret_cast<const f64x2*>(a.pred + wN + base + b * stride);
          ph[b] = *reinterpret_cast<const f64x2*>(a.pred + wN + base + b * stride + 2);
        }
        const double* rs = a.resid + wN;
        double rg[NB * V];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int e = 0; e < V; ++e) rg[b * V + e] = rs[ix[b][e]];
#pragma unroll
        for (int b = 0; b < NB; ++b) {                             // src/boot_model.rs:50-54
          d[b * V + 0] = pl[b][0] + rg[b * V + 0];
          d[b * V + 1] = pl[b][1] + rg[b * V + 1];
          d[b * V + 2] = ph[b][0] + rg[b * V + 2];
          d[b * V + 3] = ph[b][1] + rg[b * V + 3];
        }
      } else {
        f64x2 ql[NB], qh[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          ql[b] = *reinterpret_cast<const f64x2*>(a.D + dN + base + b * stride);
          qh[b] = *reinterpret_cast<const f64x2*>(a.D + dN + base + b * stride + 2);
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          d[b * V + 0] = ql[b][0];
          d[b * V + 1] = ql[b][1];
          d[b * V + 2] = qh[b][0];
          d[b * V + 3] = qh[b][1];
        }
      }
      // the candidates' dt values block by block: NC x 4 of them live at a time, not NC x all rows of the trip
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        double t[NC][V];
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int e = 0; e < V; ++e) t[c][e] = dt[c][tq[b][e]];
#pragma unroll
        for (int e = 0; e < V; ++e)
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            const double r = d[b * V + e] - ic[c] - t[c][e];
            acc[c] = acc[c] + (r * r + pen[c]);
          }
      }
    }
  };
  if constexpr (SNB > 2) blocks(std::integral_constant<int, SNB>{});  // deep loop for long rows (HBM latency) ...
  blocks(std::integral_constant<int, 2>{});                           // ... then pairs for what is left
  for (; base < N; base += stride) {                                  // remaining (possibly partial) blocks
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int i = base + e;
      if (i < N) {
        const double dd = (a.dmode == 1) ? a.pred[wN + i] + a.resid[wN + idx_row[i]] : a.D[dN + i];
        const int ti = a.tid[i];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const double r = dd - ic[c] - dt[c][ti];
          acc[c] = acc[c] + (r * r + pen[c]);
        }
      }
    }
  }
}

template <int RMAX>
__global__ __launch_bounds__(kWave, RMAX == 0 ? 1 : 2) void abn_sweep_kernel(const FitArgs a) {
  static_assert(RMAX == 0 || RMAX == -1, "0: the deep loop, -1: the pair-loop variant");
  constexpr int SNB = RMAX == 0 ? kSweepBlocks : 2;
  extern __shared__ __align__(16) double lds[];

  const int lane = threadIdx.x;
  const int dim = lane & 3;
  const long long total = (long long)a.W * a.C;
  const long long slot = (long long)blockIdx.x;
  const bool valid = slot < total;
  const long long chain = valid ? slot : 0;
  const int w = (int)(chain / a.C);
  const int j = (int)(chain - (long long)w * a.C);
  const int N = a.N, K = a.K, TP = a.TP;
  const int KP = (K + 1) & ~1;

  double* pw = lds;
  double* dtab_r = pw + kPw * TP;   // also the table of a single-candidate evaluation
  double* wconst = dtab_r + KP;     // p0uu, p0mm, eqp, eqp_weight*N
  double* dtab_e = wconst + 4;
  double* dtab_c = dtab_e + KP;

  const int wi = w * a.wstride;
  const size_t wN = (size_t)w * (size_t)N;
  const uint32_t* idx_row = (a.dmode == 1) ? a.idx + (size_t)chain * (size_t)N : nullptr;
  const size_t dN = (a.dmode == 2) ? (size_t)chain * (size_t)N : wN;  // base of this chain's rows in a.D

  if (lane == 0) {
    const double p_uu0 = a.p_uu[wi];
    wconst[0] = p_uu0;
    wconst[1] = 1.0 - p_uu0;                          // p0mm, src/ab_neutral.rs:23
    wconst[2] = a.eqp[wi];
    wconst[3] = a.eqp_w[wi] * (double)N;              // eqp_weight * nrows, src/structs.rs:210-211
  }
  __syncthreads();

  // ---- start simplex: this lane's dimension of the five vertices
  double vx[5], c[5];
  if (a.smode == 0) {
    const double* s0 = a.simplex0 + (size_t)chain * 20;
#pragma unroll
    for (int k = 0; k < 5; ++k) vx[k] = s0[4 * k + dim];
  } else {  // [params, vary() x4], src/boot_model.rs:69-75
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    const uint32_t wg = a.wid ? a.wid[w] : a.window_offset + (uint32_t)w, bg = a.boot_offset + (uint32_t)j;
    vx[0] = a.model[4 * w + dim];
#pragma unroll
    for (int v = 1; v < 5; ++v) {
      uint32_t r[4];
      philox4x32_10((uint32_t)(v - 1) * 2u + (uint32_t)(dim >> 1), bg, wg, kTagJitter, k0, k1, r);
      const uint32_t r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
      const bool odd = (dim & 1) != 0;
      vx[v] = vary_one(vx[0], odd ? r2 : r0, odd ? r3 : r1);
    }
  }

  // ---- P1 - P3 for one candidate (xd = this lane's dimension of it) into the table dt; returns the intercept and the
  // penalty term.  The one power table is free again when this returns.
  auto prepare = [&](double xd, double* dt, double& ic_out, double& pen_out) {
    const double al = dpp_mov<kDppQuadBcast0>(xd), be = dpp_mov<kDppQuadBcast1>(xd);
    const double wt = dpp_mov<kDppQuadBcast2>(xd), ic = dpp_mov<kDppQuadBcast3>(xd);
    const double p_mm = wconst[1];
    const double sv0 = wconst[0], sv1 = wt * p_mm, sv2 = (1.0 - wt) * p_mm;  // src/divergence.rs:44
    const double puu = p_uu_est(al, be);                     // src/divergence.rs:92
    const double dq = puu - wconst[2];
    ic_out = ic;
    pen_out = wconst[3] * (dq * dq);                         // src/structs.rs:210-212
    uint32_t tr = a.tri[lane < K ? lane : 0];
    if constexpr (kMatrixFma) build_power_table_mx<kWave>(al, be, a.T, lds, a.chain_stride, dt, lane);  // P1 + P2
    else build_power_table<kWave>(genmatrix(al, be), a.T, TP, pw, lane);
    __syncthreads();
#pragma unroll 1
    for (int t = lane; t < K; t += kWave) {                  // P3
      const uint32_t trn = a.tri[t + kWave < K ? t + kWave : 0];
      dt[t] = triple_dt(tr, pw, TP, sv0, sv1, sv2);
      tr = trn;
    }
    __syncthreads();
  };

  // ---- one cost evaluation, as abn_fit_kernel's stream form
  auto eval = [&](double xd) -> double {
    double ic[1], pen[1], acc[1] = {0.0};
    prepare(xd, dtab_r, ic[0], pen[0]);
    const double* const dt[1] = {dtab_r};
    sweep_rows<1, SNB>(a, lane, idx_row, wN, dN, dt, ic, pen, acc);
    const double f = group_sum_dpp<kWave>(acc[0]);
    __syncthreads();
    return f;
  };

  int st = valid ? ST_REFLECT : ST_DONE;
  int iter = 0, evals = 0;
  unsigned long long passes = 0;
  double x0 = 0.0, xr = 0.0, bx = __builtin_nan("");
  double best_cost = __builtin_inf();
  bool have_best = false;
  int fin_status = 2;

  // IterState::update() + terminate_internal() + the head of next_iter (centroid, reflection): abn_fit_kernel's
  auto begin_iteration = [&](bool count_iter) {
    const double c_best = c[0];
    if (c_best < best_cost || (__builtin_isinf(c_best) && __builtin_isinf(best_cost) &&
                               (__builtin_signbit(c_best) == __builtin_signbit(best_cost)))) {
      bx = vx[0];
      best_cost = c_best;
      have_best = true;
    }
    if (count_iter) ++iter;
    bool converged = false;
    if (!((c[4] - c[0]) > a.gap_tol)) {   // the shortcut proved in abn_fit_kernel.hpp
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < 5; ++k) sum = sum + c[k];
      const double c0 = sum / 5.0;
      double ss = 0.0;
#pragma unroll
      for (int k = 0; k < 5; ++k) ss = ss + (c[k] - c0) * (c[k] - c0);
      const double sd = __builtin_sqrt(1.0 / (5.0 - 1.0) * ss);
      converged = sd < a.sd_tol;
    }
    int status = -1;
    if (converged) status = 0;
    else if (iter >= a.max_iters) status = 1;
    else if (best_cost <= -__builtin_inf()) status = 3;
    fin_status = (status >= 0) ? (have_best ? status : 2) : fin_status;
    double acc = vx[0];
    acc = acc + vx[1];
    acc = acc + vx[2];
    acc = acc + vx[3];
    x0 = acc * (1.0 / 4.0);
    xr = x0 + (x0 - vx[4]) * 1.0;
    st = status >= 0 ? ST_DONE : ST_REFLECT;
  };

  // Solver::init: the five start costs in input order, stable sort, first termination check
#pragma unroll 1
  for (int k = 0; k < 5; ++k) {
    const double f = eval(vx[0]);
    const double tv = vx[0];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      c[q] = c[q + 1];
      vx[q] = vx[q + 1];
    }
    c[4] = f;
    vx[4] = tv;
  }
  passes += 5;
  if (valid) {
    evals = 5;
    sort5(c, vx);
    begin_iteration(false);
  }

  while (__ballot(st != ST_DONE) != 0ull) {
    // ---- the sweep: the three candidates of this iteration, one pass over the rows
    const double x_e = x0 + (xr - x0) * 2.0;        // expansion  x0 + (xr - x0) * gamma
    const double x_c = x0 + (vx[4] - x0) * 0.5;     // contraction x0 + (xw - x0) * rho
    double ic[3], pen[3], acc[3] = {0.0, 0.0, 0.0};
    prepare(xr, dtab_r, ic[0], pen[0]);
    prepare(x_e, dtab_e, ic[1], pen[1]);
    prepare(x_c, dtab_c, ic[2], pen[2]);
    const double* const dt[3] = {dtab_r, dtab_e, dtab_c};
    sweep_rows<3, SNB>(a, lane, idx_row, wN, dN, dt, ic, pen, acc);
    const double f = group_sum_dpp<kWave>(acc[0]);
    const double fe = group_sum_dpp<kWave>(acc[1]);
    const double fc = group_sum_dpp<kWave>(acc[2]);
    __syncthreads();
    passes += 1;
    // ---- decisions of NelderMead::next_iter: abn_fit_kernel's predicates on the stored costs.  fe is looked at only when
    // the expansion was asked for, fc only when the contraction was
    const bool active = st != ST_DONE;
    const bool acc_r = active && (f < c[3]) && (f >= c[0]);        // reflection accepted
    const bool go_exp = active && !acc_r && (f < c[0]);             // expansion asked for
    const bool go_con = active && !acc_r && !go_exp && (f >= c[3]);  // contraction towards the worst
    const bool nan_ref = active && !acc_r && !go_exp && !go_con;    // only reachable with a NaN cost
    const bool keep_r = go_exp && !(fe < f);                        // expansion not better: keep the reflection
    const bool acc_c = go_con && (fc < c[4]);
    const bool rej_c = go_con && !acc_c;
    const bool do_insert = acc_r || go_exp || acc_c;
    const bool start_shrink = nan_ref || (rej_c && a.shrink_variant != 0);
    const bool do_begin = do_insert || (rej_c && a.shrink_variant == 0);  // argmin 0.8.1: rejected contraction leaves the simplex
    evals += active ? ((go_exp || go_con) ? 2 : 1) : 0;
    if (rej_c && a.shrink_variant == 0 && a.no_skip == 0) {  // fixed point: finish the chain (FitArgs::no_skip)
      const int rest = a.max_iters - iter - 1;               // iterations that would repeat this one
      evals += 2 * rest;
      iter += rest;
      if (a.skipped && lane == 0 && rest > 0) atomicAdd(a.skipped, 2ull * (unsigned long long)rest);
    }
    const double xi = go_exp ? (keep_r ? xr : x_e) : (go_con ? x_c : xr);
    const double fi = go_exp ? (keep_r ? f : fe) : (go_con ? fc : f);
    if (do_insert) {
      c[4] = fi;
      vx[4] = xi;
      insert_tail<4>(c, vx);
    }
    if (do_begin) begin_iteration(true);
    // ---- NelderMead::shrink (NaN costs, or the textbook variant after a rejected contraction): one candidate per pass
    if (__ballot(start_shrink) != 0ull) {
#pragma unroll 1
      for (int k = 1; k < 5; ++k) {
        const double nv = vx[0] + (vx[1] - vx[0]) * 0.5;
        const double fk = eval(nv);
        if (start_shrink) {
          ++evals;
#pragma unroll
          for (int q = 1; q < 4; ++q) {
            c[q] = c[q + 1];
            vx[q] = vx[q + 1];
          }
          c[4] = fk;
          vx[4] = nv;
        }
      }
      passes += 4;
      if (start_shrink) {
        sort5(c, vx);
        begin_iteration(true);
      }
    }
  }

  // ---- results, as abn_fit_kernel writes them
  const double b0 = dpp_mov<kDppQuadBcast0>(bx), b1 = dpp_mov<kDppQuadBcast1>(bx);
  if (valid) {
    if (lane < 4) a.best[(size_t)chain * 4 + lane] = bx;
    if (lane == 0) {
      FitInfoDev fo;
      fo.best_cost = best_cost;
      fo.iters = iter;
      fo.evals = evals;
      fo.status = fin_status;
      fo.lanes = kWave | ((kStreamVec - 1) << 8);  // reduction-order code (oracle: `lanes`)
      a.info[chain] = fo;
      if (a.passes) atomicAdd(a.passes, passes);
    }
    if (a.raw) {
      double* ro = a.raw + (size_t)chain * 7;
      if (lane < 4) ro[lane] = bx;
      if (lane == 4) ro[4] = est_mm(b0, b1);
      if (lane == 5) ro[5] = est_um(b0, b1);
      if (lane == 6) ro[6] = p_uu_est(b0, b1);
    }
  }
}

}  // namespace abn
