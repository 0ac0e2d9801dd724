// simulate.hpp — `alphabeta --simulate`: the pedigree of methylomes simulated on the device under the ABneutral model
// (src/divergence.rs:33-114 run forwards; csrc/abn_sim.hpp) in the place of Pedigree::build (src/pedigree.rs:92-193).  The
// nodelist and the edgelist give the tree; no methylome file is opened.
#pragma once

#include "pedigree_build.hpp"

namespace alphabeta {
namespace simulate {

struct Request {  // --simulate ALPHA,BETA --sim-sites L [--sim-p0uu P] [--sim-weight W]
  bool wanted = false;
  double alpha = 0.0, beta = 0.0;
  double p_uu0 = 0.75, weight = 0.5;
  long long sites = 0;
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

}  // namespace simulate
}  // namespace alphabeta
