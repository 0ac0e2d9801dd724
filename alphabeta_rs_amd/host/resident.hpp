// resident.hpp — what the host layer builds from RESIDENT methylomes (windows::ResidentSites: a methylome parsed on the
// device and left there), written once for its three drivers — metaprofile::extract_in_memory (metaprofile.hpp),
// detail::read_inputs_resident (below, behind `alphabeta --sites device`) and metaprofile::alphabeta_multiple_tiles
// (tiles.hpp): the loader, the three --align modes as one table of the library's create calls, what an alignment made of
// every sample and the line that says so.  Included at the end of windows_extract.hpp.
#pragma once

#include "windows_extract.hpp"

namespace alphabeta {
namespace resident {

inline std::string base_name(const std::string& p) {
  const size_t slash = p.find_last_of('/');
  return p.substr(slash == std::string::npos ? 0 : slash + 1);
}

inline std::vector<abn_sites*> pointers(const std::vector<windows::ResidentSites>& sites) {
  std::vector<abn_sites*> out;
  for (const auto& s : sites) out.push_back(s.get());
  return out;
}

// The samples' methylomes in the order added, each parsed as it comes and its text dropped.  skip_lines: 1 passes over the
// header row as Windows::extract does (src/windows.rs:303-306), 0 reads every line as the pedigree build does
// (src/pedigree.rs:147-163); the invalid-status warnings appear in file order either way.
struct Samples {
  Device& dev;
  size_t skip_lines;
  std::vector<windows::ResidentSites> sites;
  void add_text(const std::string& text) { sites.push_back(windows::parse_sites_resident(dev, text, skip_lines)); }
  void add_file(const std::string& path) {  // a sampled node's file (src/pedigree.rs:147-150)
    if (!std::ifstream(path)) throw Error(ABN_ERR_INVALID_ARG, "Could not open node file: " + path);
    add_text(detail::read_file(path, "methylome"));
  }
  std::vector<abn_sites*> pointers() const { return resident::pointers(sites); }
};

// One row per Align, indexed by its value: the create call for windows and for codes with the name Device::check puts into
// an error's text, the call that reports what the alignment did, and the two ends of the per-sample line.
struct AlignMode {
  decltype(&abn_windows_create_parsed) windows_create;
  const char* windows_name;
  decltype(&abn_windows_common) windows_counts;
  decltype(&abn_codes_create_parsed) codes_create;
  const char* codes_name;
  decltype(&abn_codes_common) codes_counts;
  const char *says, *of_them;  // null: nothing to say
};
inline const AlignMode& align_mode(Align a) {
  static const AlignMode modes[3] = {
      {abn_windows_create_parsed, "abn_windows_create_parsed", abn_windows_common, abn_codes_create_parsed,
       "abn_codes_create_parsed", abn_codes_common, nullptr, nullptr},
      {abn_windows_create_aligned, "abn_windows_create_aligned", abn_windows_common, abn_codes_create_aligned,
       "abn_codes_create_aligned", abn_codes_common, "Aligned by position: ", " kept"},
      {abn_windows_create_union, "abn_windows_create_union", abn_windows_union, abn_codes_create_union,
       "abn_codes_create_union", abn_codes_union, "Aligned by union: ", " in the union"}};
  return modes[(int32_t)a];
}

// What an alignment made of the samples: every sample's sites as they came, and the sites each has now (Position: those
// every sample keeps; Union: those any sample holds)
struct AlignCounts {
  std::vector<int64_t> before;
  int64_t n = -1;
};
inline AlignCounts align_counts(const windows::Handle& h, Align a) {
  AlignCounts c;
  c.before.resize(h.n_samples());
  align_mode(a).windows_counts(h.get(), c.before.data(), &c.n, nullptr);
  return c;
}
inline AlignCounts align_counts(const abn_codes* h, size_t n_samples, Align a) {
  AlignCounts c;
  c.before.resize(n_samples);
  align_mode(a).codes_counts(h, c.before.data(), &c.n, nullptr);
  return c;
}
inline AlignCounts align_counts(const abn_tiles* h, const std::vector<windows::ResidentSites>& sites) {
  AlignCounts c;
  for (const auto& s : sites) c.before.push_back((int64_t)s.size());
  abn_tiles_info(h, nullptr, &c.n, nullptr, nullptr, nullptr);  // the tiles' columns
  return c;
}

// One line per sample, each with its '\n'; none without an alignment
inline std::vector<std::string> align_report(Align a, const std::vector<std::string>& names, const AlignCounts& c) {
  std::vector<std::string> lines;
  const AlignMode& m = align_mode(a);
  for (size_t s = 0; m.says && s < names.size(); ++s)
    lines.push_back(m.says + names[s] + ": " + std::to_string(c.before[s]) + " sites, " + std::to_string(c.n) + m.of_them + "\n");
  return lines;
}

}  // namespace resident

namespace windows {
inline Handle::Handle(Device& dev, const abn_windows_params& p, const Genome& genome, const GeneRule& rule,
                      double posterior_max_filter, const std::vector<ResidentSites>& samples, Align align)
    : n_(samples.size()) {
  const GenesHandle genes(dev, genome);
  const abn_gene_rule r{rule.cutoff, rule.cutoff_gene_length ? 1 : 0};
  const resident::AlignMode& m = resident::align_mode(align);
  dev.check(m.windows_create(dev.get(), &p, genes.get(), &r, posterior_max_filter, (int32_t)n_, resident::pointers(samples).data(),
                             h_.out()),
            m.windows_name);
  fetch();
}
}  // namespace windows

namespace detail {
inline Inputs read_inputs_resident(const std::string& nodelist, const std::string& edgelist, double posterior_max_filter,
                                   std::vector<double>& dm, const std::vector<std::string>* texts, Align align) {
  Inputs in = read_graph(nodelist, edgelist);
  std::vector<Node>& nodes = in.nodes;
  const size_t nn = nodes.size();
  if (texts && texts->size() != nn) throw Error(ABN_ERR_INVALID_ARG, "one text per sampled node");
  Device& dev = default_device();
  resident::Samples samples{dev, /*skip_lines=*/0, {}};
  std::vector<std::string> names;
  for (size_t i = 0; i < nn; ++i) {
    names.push_back(nodes[i].file);
    if (texts) samples.add_text((*texts)[i]);
    else samples.add_file(nodes[i].file);
  }
  Owned<abn_codes, abn_codes_destroy> codes;
  int32_t same_len = 1;
  if (nn > 0) {
    const resident::AlignMode& m = resident::align_mode(align);
    dev.check(m.codes_create(dev.get(), posterior_max_filter, (int32_t)nn, samples.pointers().data(), codes.out()), m.codes_name);
    for (const std::string& line : resident::align_report(align, names, resident::align_counts(codes.get(), nn, align)))
      diag_printf("%s", line.c_str());
    resident_build_calls().fetch_add(1, std::memory_order_relaxed);
    std::vector<double> sum(nn);
    std::vector<int64_t> kept(nn);
    abn_codes_stats(codes.get(), nullptr, sum.data(), kept.data());
    abn_codes_info(codes.get(), nullptr, nullptr, nullptr, &same_len);
    abn_codes_kernel_ms(codes.get(), resident_kernel_ms());
    for (size_t i = 0; i < nn; ++i) nodes[i].rc_meth_lvl = sum[i] / (double)kept[i];  // :165-166
  }
  fold_p0uu(in);
  if (same_len && nn >= 2) {
    std::vector<double> dv(nn * (nn - 1) / 2);
    dev.check(abn_codes_pairwise(codes.get(), nullptr, nullptr, dv.data()), "Pedigree::build (pairwise divergence)");
    dm = dmatrix_of_pairs(nn, dv.data());
    return in;
  }
  // the reference's answer for samples of different length is per pair (:221-227): the host loop gives it
  for (size_t i = 0; i < nn; ++i) {
    const windows::ResidentSites& mine = samples.sites[i];
    const size_t n = mine.size();
    std::vector<double> pm(n), ml(n);
    std::vector<uint8_t> status(n);
    dev.check(abn_sites_fetch(mine.get(), nullptr, nullptr, nullptr, nullptr, nullptr, pm.data(), status.data(), nullptr, ml.data()),
              "abn_sites_fetch");
    nodes[i].sites.resize(n);
    for (size_t k = 0; k < n; ++k) nodes[i].sites[k] = Site{pm[k], status[k], ml[k]};
  }
  dm = dmatrix_on_host(in, posterior_max_filter);
  return in;
}
}  // namespace detail
}  // namespace alphabeta
