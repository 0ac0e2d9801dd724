// simulate.hpp — `alphabeta --simulate`: the pedigree of methylomes simulated on the device under the ABneutral model
// (src/divergence.rs:33-114 run forwards; csrc/abn_sim.hpp) in the place of Pedigree::build (src/pedigree.rs:92-193).  The
// nodelist and the edgelist give the tree; no methylome file is opened.  With --sim-replicates R the run is a replicate study
// (abn_sim_study): R pedigrees as the column ranges of one simulation, observed through miscalls and dropouts where asked
// for, all of them the windows of ONE plan (n_starts = S, n_boot = 0, window id = the replicate), as the block bootstrap
// fits its rows (block_bootstrap.hpp); replicate 0 is the run's usual pedigree.
#pragma once

#include "block_bootstrap.hpp"
#include "pedigree_build.hpp"

namespace alphabeta {
namespace simulate {

struct Request {  // --simulate ALPHA,BETA --sim-sites L [--sim-p0uu P] [--sim-weight W]
  bool wanted = false;
  double alpha = 0.0, beta = 0.0;
  double p_uu0 = 0.75, weight = 0.5;
  long long sites = 0;
  // [--sim-replicates R [--sim-starts S] [--sim-miscall E] [--sim-dropout F]]
  long long replicates = 0;  // 0: one pedigree, no study
  int starts = metaprofile::kBlockStartsDefault;
  double miscall = 0.0, dropout = 0.0;
};

// "A,B" -> two numbers
inline bool parse_rates(const std::string& text, double& alpha, double& beta) {
  const auto parts = detail::split_any(text, ",");
  return parts.size() == 2 && detail::parse_f64(parts[0], alpha) && detail::parse_f64(parts[1], beta);
}
constexpr const char* kSimulateExpects = "--simulate expects ALPHA,BETA, two rates in [0, 1]";

// The tree of a nodelist and an edgelist, numbered breadth-first from the root, children in the edgelist's order
struct Tree {
  std::vector<int32_t> parent, generation;
  std::vector<uint8_t> emit;
  std::vector<std::string> name;
};
inline Tree read_tree(const std::string& nodelist, const std::string& edgelist) {
  const detail::Inputs in = detail::read_graph(nodelist, edgelist);
  const size_t V = in.all.size();
  for (size_t a = 0; a < V; ++a)
    for (size_t b = a + 1; b < V; ++b)
      if (in.all[a].name == in.all[b].name) throw Error(ABN_ERR_BAD_PEDIGREE, "--simulate: node " + in.all[a].name + " is listed twice");
  std::vector<size_t> incoming(V, 0);
  std::vector<std::vector<size_t>> children(V);
  for (const auto& e : in.edges) {
    ++incoming[e.to];
    children[e.from].push_back(e.to);
  }
  size_t root = V;
  for (size_t v = 0; v < V; ++v) {
    if (incoming[v] > 1) throw Error(ABN_ERR_BAD_PEDIGREE, "--simulate: node " + in.all[v].name + " has more than one incoming edge: not a tree");
    if (incoming[v] == 0) {
      if (root != V) throw Error(ABN_ERR_BAD_PEDIGREE, "--simulate: nodes " + in.all[root].name + " and " + in.all[v].name + " both have no incoming edge: not one tree");
      root = v;
    }
  }
  if (root == V) throw Error(ABN_ERR_BAD_PEDIGREE, "--simulate: no node without an incoming edge: not a tree");
  Tree t;
  std::vector<size_t> order{root};  // file indices in breadth-first order
  t.parent.push_back(-1);
  for (size_t at = 0; at < order.size(); ++at)
    for (size_t child : children[order[at]]) {
      order.push_back(child);
      t.parent.push_back((int32_t)at);
    }
  if (order.size() != V) throw Error(ABN_ERR_BAD_PEDIGREE, "--simulate: a cycle apart from the root's tree: not a tree");
  for (size_t v : order) {
    t.generation.push_back((int32_t)std::min<uint32_t>(in.all[v].generation, 0x7fffffffu));
    t.emit.push_back(in.all[v].meth ? 1 : 0);
    t.name.push_back(in.all[v].name);
  }
  return t;
}

// Pedigree::build of the simulated methylomes: (rows, p0uu) of abn_sim_pedigree
inline std::pair<Pedigree, double> build(const Request& rq, const std::string& nodelist, const std::string& edgelist, uint64_t seed) {
  const Tree t = read_tree(nodelist, edgelist);
  const int32_t V = (int32_t)t.parent.size();
  std::vector<uint64_t> thr((size_t)V * 6);
  char text[256];
  if (int rc = abn_sim_thresholds(rq.alpha, rq.beta, rq.p_uu0, rq.weight, V, t.parent.data(), t.generation.data(), thr.data(), text,
                                  (int32_t)sizeof text))
    throw Error(rc, std::string("--simulate: ") + text);
  size_t n = 0;
  for (uint8_t e : t.emit) n += e;
  const size_t pairs = n * (n > 0 ? n - 1 : 0) / 2;
  std::vector<double> rows(std::max<size_t>(pairs, 1) * 4);
  double p0uu = 0.0;
  Device& dev = default_device();
  dev.check(abn_sim_pedigree(dev.get(), seed, V, t.parent.data(), t.generation.data(), thr.data(), t.emit.data(), rq.sites,
                             rows.data(), &p0uu, nullptr),
            "--simulate");
  Pedigree ped;
  for (size_t r = 0; r < pairs; ++r) ped.push_row(rows[4 * r], rows[4 * r + 1], rows[4 * r + 2], rows[4 * r + 3]);
  return {std::move(ped), p0uu};
}

// A replicate study: simulation.txt and simulation_raw.npy beside the run's usual files
struct Study {
  Pedigree pedigree;  // replicate 0
  double p0uu = 0.0;
  std::string txt;    // simulation.txt
  RawAnalysis raw;    // simulation_raw.npy: (R, 7) with the columns of raw.npy, NaN rows for the replicates left out
  size_t ok = 0;
};

inline std::string study_header() {
  return "alpha_true;beta_true;sites;replicates;replicates_ok;mean_alpha;mean_beta;sd_alpha;sd_beta;ci_alpha_0.025;ci_alpha_0.975;ci_beta_0.025;"
         "ci_beta_0.975\n";
}

// `why` or "": R L within what one simulation draws (the counter word holds (R L) >> 2)
inline std::string study_refusal(const Request& rq) {
  if (rq.replicates < 1) return "--sim-replicates expects a positive number of replicates";
  if (rq.replicates > 0x7fffffffLL || rq.sites > (1ll << 34) / rq.replicates)
    return "--sim-replicates x --sim-sites lies above 2^34 sites, what one simulation draws";
  if (rq.starts < 1) return "--sim-starts expects a positive number of starts";
  if (!(rq.miscall >= 0.0 && rq.miscall <= 1.0)) return "--sim-miscall expects a probability in [0, 1]";
  if (!(rq.dropout >= 0.0 && rq.dropout <= 1.0)) return "--sim-dropout expects a probability in [0, 1]";
  return "";
}

inline Study study(const Request& rq, const std::string& nodelist, const std::string& edgelist, uint64_t seed) {
  const Tree t = read_tree(nodelist, edgelist);
  const int32_t V = (int32_t)t.parent.size();
  std::vector<uint64_t> thr((size_t)V * 6);
  char text[256];
  if (int rc = abn_sim_thresholds(rq.alpha, rq.beta, rq.p_uu0, rq.weight, V, t.parent.data(), t.generation.data(), thr.data(), text,
                                  (int32_t)sizeof text))
    throw Error(rc, std::string("--simulate: ") + text);
  uint64_t othr[9];
  const bool noisy = rq.miscall > 0.0 || rq.dropout > 0.0;  // at 0 / 0 no observation kernel runs
  if (noisy) {
    const double e = rq.miscall, h = 0.5 * rq.miscall, f = rq.dropout;
    const double miscall[9] = {1.0 - e, h, h, h, 1.0 - e, h, h, h, 1.0 - e}, dropout[3] = {f, f, f};
    if (int rc = abn_sim_obs_thresholds(miscall, dropout, othr, text, (int32_t)sizeof text))
      throw Error(rc, std::string("--simulate: ") + text);
  }
  size_t n = 0;
  for (uint8_t e : t.emit) n += e;
  const size_t P = n * (n > 0 ? n - 1 : 0) / 2, R = (size_t)rq.replicates;
  std::vector<double> times(std::max<size_t>(P, 1) * 3), D(std::max<size_t>(R * P, 1)), p0uu(R);
  Device& dev = default_device();
  dev.check(abn_sim_study(dev.get(), seed, V, t.parent.data(), t.generation.data(), thr.data(), t.emit.data(), noisy ? othr : nullptr,
                          rq.sites, (int32_t)R, times.data(), D.data(), p0uu.data(), nullptr, nullptr),
            "--simulate");
  Study out;
  for (size_t i = 0; i < P; ++i) out.pedigree.push_row(times[3 * i], times[3 * i + 1], times[3 * i + 2], D[i]);
  out.p0uu = p0uu[0];

  const double nan = std::nan("");
  auto finite_row = [](const double* p, size_t count) {
    for (size_t c = 0; c < count; ++c)
      if (!std::isfinite(p[c])) return false;
    return true;
  };
  std::vector<size_t> wins;  // the replicates that are a finite pedigree
  for (size_t r = 0; r < R; ++r)
    if (std::isfinite(p0uu[r]) && finite_row(&D[r * P], P)) wins.push_back(r);
  std::vector<double> model(R * 4, nan);
  if (!wins.empty() && P > 0) {
    const size_t W = wins.size();
    std::vector<double> Dw(W * P), pw(W), mod(W * 4);
    std::vector<uint32_t> ids(W);
    std::vector<int32_t> best(W);
    for (size_t v = 0; v < W; ++v) {
      std::copy(D.begin() + (std::ptrdiff_t)(wins[v] * P), D.begin() + (std::ptrdiff_t)((wins[v] + 1) * P), Dw.begin() + (std::ptrdiff_t)(v * P));
      pw[v] = p0uu[wins[v]];
      ids[v] = (uint32_t)wins[v];
    }
    Owned<abn_plan, abn_plan_destroy> plan;
    dev.check(abn_plan_create(dev.get(), &dev.options, times.data(), (int32_t)P, (int32_t)W, rq.starts, 0, 0, 0, plan.out()),
              "abn_plan_create");
    dev.check(abn_plan_set_window_ids(plan.get(), ids.data()), "abn_plan_set_window_ids");
    dev.check(abn_plan_set_windows(plan.get(), Dw.data(), pw.data(), nullptr, nullptr), "abn_plan_set_windows");
    dev.check(abn_plan_run(plan.get()), "abn_plan_run");
    int rc = abn_plan_download(plan.get(), mod.data(), nullptr, nullptr, nullptr, nullptr, nullptr, best.data());
    if (rc == ABN_ERR_NO_FINITE_FIT) rc = ABN_OK;  // per replicate below
    dev.check(rc, "simulation study plan");
    for (size_t v = 0; v < W; ++v)
      if (best[v] >= 0) std::copy(mod.begin() + (std::ptrdiff_t)(4 * v), mod.begin() + (std::ptrdiff_t)(4 * v + 4), model.begin() + (std::ptrdiff_t)(4 * wins[v]));
  }
  std::vector<size_t> fitted;  // the replicates with a finite fit
  std::vector<double> best4;
  for (size_t r = 0; r < R; ++r) {
    if (!finite_row(&model[r * 4], 4)) continue;
    fitted.push_back(r);
    best4.insert(best4.end(), &model[r * 4], &model[r * 4] + 4);
  }
  std::vector<double> table(fitted.size() * 7), kept_rows;
  if (!fitted.empty())
    dev.check(abn_bootstrap_rows(dev.get(), best4.data(), (int64_t)fitted.size(), table.data()), "abn_bootstrap_rows");
  out.raw.rows.assign(R * 7, nan);
  out.raw.n_boot = R;
  for (size_t k = 0; k < fitted.size(); ++k) {
    if (!finite_row(&table[k * 7], 7)) continue;  // a NaN row is left out too
    kept_rows.insert(kept_rows.end(), table.begin() + (std::ptrdiff_t)(k * 7), table.begin() + (std::ptrdiff_t)(k * 7 + 7));
    std::copy(table.begin() + (std::ptrdiff_t)(k * 7), table.begin() + (std::ptrdiff_t)(k * 7 + 7), out.raw.rows.begin() + (std::ptrdiff_t)(fitted[k] * 7));
    ++out.ok;
  }
  double a[32];
  std::fill(a, a + 32, nan);
  if (out.ok > 0 && abn_analyze(kept_rows.data(), (int64_t)out.ok, a) != ABN_OK) std::fill(a, a + 32, nan);
  out.txt = study_header() + fmt_f64(rq.alpha) + ";" + fmt_f64(rq.beta) + ";" + std::to_string(rq.sites) + ";" + std::to_string(R) + ";" +
            std::to_string(out.ok) + ";" + fmt_f64(a[0]) + ";" + fmt_f64(a[1]) + ";" + fmt_f64(a[8]) + ";" + fmt_f64(a[9]) + ";" +
            fmt_f64(a[16]) + ";" + fmt_f64(a[24]) + ";" + fmt_f64(a[17]) + ";" + fmt_f64(a[25]) + "\n";
  return out;
}

}  // namespace simulate
}  // namespace alphabeta
