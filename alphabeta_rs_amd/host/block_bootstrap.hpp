// block_bootstrap.hpp — the block bootstrap of pooled and genome-wide rates (`metaprofile_alphabeta --block-bootstrap R
// [--block-starts S]`, csrc/abn_blocks.hpp): the uncertainty of a rate estimated for a pool of regions or a tiled genome,
// where the reference has only the residual bootstrap of one pedigree's rows (src/boot_model.rs:43-57).  The handle's
// blocks — a pool's merged segments, the fixed tiles of a genome — are drawn with replacement on the device
// (abn_tiles_block_bootstrap), R replicates and the identity row per group; every row (group, r) is then a pedigree of its
// own: p0uu* by the fold of window_from_handle over level* / kept*, the rows from detail::convert_times and dvalue*.  All
// rows of all groups share the topology and are the windows of ONE plan (n_starts = S, n_boot = 0) whose window id is
// (group << 20) | r, r = 2^20 - 1 for the identity row, so a row's random streams depend on neither R nor the number of
// groups.  Per group the replicates with finite D, a finite fit and a finite table row go through abn_bootstrap_rows and
// abn_analyze; the others are left out and counted.
#pragma once

#include "metaprofile.hpp"

namespace alphabeta {
namespace metaprofile {

constexpr uint32_t kBlockIdentityRow = (1u << 20) - 1;  // the identity row's id inside its group
constexpr int kBlockStartsDefault = 10;                 // BASELINE C3's start count: a choice, not a measurement

struct BlockBootstrap {
  size_t replicates = 0, groups = 0;
  std::string txt;          // block_bootstrap.txt
  std::vector<double> raw;  // block_raw.npy: (replicates, 7, groups) C order, NaN rows for the replicates left out
};

inline std::string block_bootstrap_header() {
  return "group;name;blocks;replicates;replicates_ok;alpha;beta;sd_alpha;sd_beta;ci_alpha_0.025;ci_alpha_0.975;ci_beta_0.025;"
         "ci_beta_0.975\n";
}

// names: the groups' names (the pools', or "genome"); times, sample_of, n_samples as window_from_handle takes them
inline BlockBootstrap block_bootstrap(abn_tiles* th, const std::vector<std::string>& names,
                                      const std::vector<detail::PairTimes>& times, const std::vector<size_t>& sample_of,
                                      size_t n_samples, int64_t n_replicates, int n_starts) {
  Device& dev = default_device();
  const double nan = std::nan("");
  int64_t n_groups = 0;
  dev.check(abn_tiles_block_groups(th, &n_groups, nullptr, nullptr, nullptr), "abn_tiles_block_groups");
  const size_t G = (size_t)n_groups, R = (size_t)n_replicates, rows = R + 1, W = G * rows, n = n_samples, P = n * (n - 1) / 2;
  if (G != names.size()) throw Error(ABN_ERR_INVALID_ARG, "the block bootstrap's groups are not the run's");
  std::vector<int64_t> gb(G), ge(G);
  dev.check(abn_tiles_block_groups(th, nullptr, nullptr, gb.data(), ge.data()), "abn_tiles_block_groups");
  std::vector<double> dv(std::max<size_t>(W * P, 1), 0.0), level(W * n);
  std::vector<int64_t> kept(W * n);
  dev.check(abn_tiles_block_bootstrap(th, dev.options.seed, n_replicates, nullptr, nullptr, dv.data(), level.data(), kept.data()),
            "abn_tiles_block_bootstrap");
  // window_from_handle reads [sample][window]; a window here is a row (group, r)
  std::vector<double> level_of(n * W);
  std::vector<int64_t> kept_of(n * W);
  for (size_t w = 0; w < W; ++w)
    for (size_t s = 0; s < n; ++s) level_of[s * W + w] = level[w * n + s], kept_of[s * W + w] = kept[w * n + s];

  std::vector<Win> wins;  // the rows that are a finite pedigree; Win::index = the row
  for (size_t w = 0; w < W; ++w) {
    try {
      Win win = window_from_handle(names[w / rows], w, times, sample_of, n, W, w, level_of, kept_of, &dv[w * P]);
      bool finite = std::isfinite(win.p0uu);
      for (size_t i = 0; i < win.ped.nrows(); ++i) finite = finite && std::isfinite(win.ped.at(i, 3));
      if (finite) wins.push_back(std::move(win));
    } catch (const Error&) {  // an empty pedigree: the row is left out
    }
  }
  std::vector<double> model(W * 4, nan);  // every row's fitted model; NaN: left out, or no finite fit
  if (!wins.empty()) {
    const size_t N = wins[0].ped.nrows(), V = wins.size();
    std::vector<double> gens(N * 3), D(V * N), p0uu(V), mod(V * 4);
    std::vector<uint32_t> ids(V);
    std::vector<int32_t> best(V);
    for (size_t i = 0; i < N; ++i)
      for (size_t c = 0; c < 3; ++c) gens[i * 3 + c] = wins[0].ped.at(i, c);
    for (size_t v = 0; v < V; ++v) {
      const size_t g = wins[v].index / rows, r = wins[v].index % rows;
      for (size_t i = 0; i < N; ++i) D[v * N + i] = wins[v].ped.at(i, 3);
      p0uu[v] = wins[v].p0uu;
      ids[v] = ((uint32_t)g << 20) | (r == R ? kBlockIdentityRow : (uint32_t)r);
    }
    Owned<abn_plan, abn_plan_destroy> plan;
    dev.check(abn_plan_create(dev.get(), &dev.options, gens.data(), (int32_t)N, (int32_t)V, n_starts, 0, 0, 0, plan.out()),
              "abn_plan_create");
    dev.check(abn_plan_set_window_ids(plan.get(), ids.data()), "abn_plan_set_window_ids");
    dev.check(abn_plan_set_windows(plan.get(), D.data(), p0uu.data(), nullptr, nullptr), "abn_plan_set_windows");
    dev.check(abn_plan_run(plan.get()), "abn_plan_run");
    int rc = abn_plan_download(plan.get(), mod.data(), nullptr, nullptr, nullptr, nullptr, nullptr, best.data());
    if (rc == ABN_ERR_NO_FINITE_FIT) rc = ABN_OK;  // per row below
    dev.check(rc, "block bootstrap plan");
    for (size_t v = 0; v < V; ++v)
      if (best[v] >= 0) std::copy(mod.begin() + (std::ptrdiff_t)(4 * v), mod.begin() + (std::ptrdiff_t)(4 * v + 4), model.begin() + (std::ptrdiff_t)(4 * wins[v].index));
  }

  BlockBootstrap out;
  out.replicates = R, out.groups = G;
  out.raw.assign(R * 7 * G, nan);
  out.txt = block_bootstrap_header();
  auto finite_row = [](const double* p, size_t count) {
    for (size_t c = 0; c < count; ++c)
      if (!std::isfinite(p[c])) return false;
    return true;
  };
  for (size_t g = 0; g < G; ++g) {
    std::vector<size_t> fitted;  // the replicates with a finite fit
    std::vector<double> best4;
    for (size_t r = 0; r < R; ++r) {
      const double* m = &model[(g * rows + r) * 4];
      if (!finite_row(m, 4)) continue;
      fitted.push_back(r);
      best4.insert(best4.end(), m, m + 4);
    }
    std::vector<double> table(fitted.size() * 7), kept_rows;
    if (!fitted.empty())
      dev.check(abn_bootstrap_rows(dev.get(), best4.data(), (int64_t)fitted.size(), table.data()), "abn_bootstrap_rows");
    size_t ok = 0;
    for (size_t k = 0; k < fitted.size(); ++k) {
      if (!finite_row(&table[k * 7], 7)) continue;  // a NaN row is left out too
      kept_rows.insert(kept_rows.end(), table.begin() + (std::ptrdiff_t)(k * 7), table.begin() + (std::ptrdiff_t)(k * 7 + 7));
      for (size_t c = 0; c < 7; ++c) out.raw[(fitted[k] * 7 + c) * G + g] = table[k * 7 + c];
      ++ok;
    }
    double a[32];
    std::fill(a, a + 32, nan);
    if (ok > 0 && abn_analyze(kept_rows.data(), (int64_t)ok, a) != ABN_OK) std::fill(a, a + 32, nan);
    const double* identity = &model[(g * rows + R) * 4];  // alpha and beta of the observed data
    out.txt += std::to_string(g) + ";" + names[g] + ";" + std::to_string(ge[g] - gb[g]) + ";" + std::to_string(R) + ";" +
               std::to_string(ok) + ";" + fmt_f64(identity[0]) + ";" + fmt_f64(identity[1]) + ";" + fmt_f64(a[8]) + ";" +
               fmt_f64(a[9]) + ";" + fmt_f64(a[16]) + ";" + fmt_f64(a[24]) + ";" + fmt_f64(a[17]) + ";" + fmt_f64(a[25]) + "\n";
  }
  return out;
}

// block_raw.npy: (replicates, 7, groups), '<f8'
inline void write_block_raw_npy(const BlockBootstrap& b, const std::string& path) {
  Output o;
  o.raw = b.raw;
  o.iterations = b.replicates;
  o.n_ok = b.groups;
  write_raw_npy(o, path);
}

}  // namespace metaprofile
}  // namespace alphabeta
