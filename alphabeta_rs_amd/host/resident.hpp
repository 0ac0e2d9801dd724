// resident.hpp — what the host layer builds from RESIDENT methylomes (windows::ResidentSites: a methylome parsed on the
// device and left there), written once for its three drivers — metaprofile::extract_in_memory (metaprofile.hpp),
// detail::read_inputs_resident (below, behind `alphabeta --sites device`) and metaprofile::alphabeta_multiple_tiles
// (tiles.hpp): the loader, the three --align modes as one table of the library's create calls, what an alignment made of
// every sample and the line that says so.  Included at the end of windows_extract.hpp.
#pragma once

#include <array>

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
// contexts: the methylation contexts whose lines are sites (1 CG, 2 CHG, 4 CHH; the reference reads CG alone).  Under
// several, every methylome is still read and parsed once: split() partitions each on the device (abn_sites_split) and hands
// out one handle set per context, each what a load under that context alone would hold.
// sort (--sort): each methylome, parsed and its deferred lines inserted as ever — the warnings name the file's own lines —
// is then sorted by genomic position on the device (abn_sites_sort) and the parent dropped: only the sorted handle is
// kept, and a split of it is sorted too (the split is stable).  sort_report gets one line, with its '\n', per sample that
// had a descent; the driver prints them next to the alignment report.
// dedup (--dedup POLICY; -1: none): implies the sort; the sorted methylome is then collapsed on the device (abn_sites_dedup:
// every run of equal keys to at most one record) and the sorted handle dropped, so a split is of the collapsed sites — unless
// the sort's info says there is nothing to collapse: its equal neighbours are those of its INPUT, so they are the sorted
// handle's only for an input without a descent, and a sample that was out of order is collapsed to find out (without a
// repeated key the sorted handle is kept).  sort_report gets one more line per sample that held repeats, behind the sort's.
constexpr const char* kDedupNames[4] = {"first", "last", "best", "drop"};  // ABN_DEDUP_FIRST .. ABN_DEDUP_DROP
constexpr const char* kDedupExpects = "--dedup expects one of first, last, best, drop";
// "best" -> ABN_DEDUP_BEST; -1: no policy's name
inline int parse_dedup(const std::string& name) {
  for (int p = 0; p < 4; ++p)
    if (name == kDedupNames[p]) return p;
  return -1;
}

struct Samples {
  Device& dev;
  size_t skip_lines;
  std::vector<windows::ResidentSites> sites;
  unsigned contexts = 1u;
  bool sort = false;
  int dedup = -1;
  std::vector<std::string> sort_report;
  void add_text(const std::string& text, const std::string& name = std::string()) {
    windows::ResidentSites parsed = windows::parse_sites_resident(dev, text, skip_lines, /*slab_bytes=*/0, contexts);
    if (!sort && dedup < 0) {
      sites.push_back(std::move(parsed));
      return;
    }
    abn_sites* sorted = nullptr;
    dev.check(abn_sites_sort(parsed.get(), &sorted), "abn_sites_sort");
    sites.emplace_back(sorted);
    int64_t info[4] = {0, 0, 0, 0};
    dev.check(abn_sites_sort_info(sorted, info, nullptr), "abn_sites_sort_info");
    if (info[1] > 0)
      sort_report.push_back("Sorted by position: " + name + ": " + std::to_string(info[0]) + " sites, " + std::to_string(info[1]) +
                            " descents\n");
    if (dedup < 0 || (info[1] == 0 && info[2] == 0)) return;  // in order and no equal neighbours: nothing to collapse
    abn_sites* made = nullptr;
    dev.check(abn_sites_dedup(sorted, dedup, &made), "abn_sites_dedup");
    windows::ResidentSites collapsed(made);
    dev.check(abn_sites_dedup_info(made, info, nullptr), "abn_sites_dedup_info");
    if (info[2] == 0) return;  // no repeated key: the sorted handle stays
    sites.back() = std::move(collapsed);
    sort_report.push_back("Collapsed repeated sites: " + name + ": " + std::to_string(info[0]) + " sites, " +
                          std::to_string(info[0] - info[1]) + " removed in " + std::to_string(info[2]) + " repeated keys, " +
                          std::to_string(info[3]) + " disagreeing (" + kDedupNames[dedup] + ")\n");
  }
  // a sampled node's file (src/pedigree.rs:147-150); name: what the sort's line calls it
  void add_file(const std::string& path, const std::string& name = std::string()) {
    if (!std::ifstream(path)) throw Error(ABN_ERR_INVALID_ARG, "Could not open node file: " + path);
    add_text(detail::read_file(path, "methylome"), name.empty() ? path : name);
  }
  std::vector<abn_sites*> pointers() const { return resident::pointers(sites); }
  // [c] = every sample's sites of context c, in the samples' order; empty for a context outside the mask
  std::array<std::vector<windows::ResidentSites>, 3> split() const {
    std::array<std::vector<windows::ResidentSites>, 3> out;
    for (const auto& s : sites) {
      abn_sites* kids[3] = {nullptr, nullptr, nullptr};
      const int rc = abn_sites_split(s.get(), kids);
      for (int c = 0; c < 3; ++c)
        if (kids[c]) out[(size_t)c].emplace_back(kids[c]);
      dev.check(rc, "abn_sites_split");
    }
    return out;
  }
};

constexpr const char* kContextNames[3] = {"CG", "CHG", "CHH"};
constexpr const char* kContextsExpects = "--contexts expects a comma-separated list of distinct names of CG, CHG, CHH";
// "CG,CHH" -> 5; false: an unknown or repeated name, or none
inline bool parse_contexts(const std::string& list, unsigned& mask) {
  mask = 0;
  for (const std::string& name : detail::split_any(list, ",")) {
    int c = 0;
    while (c < 3 && name != kContextNames[c]) ++c;
    if (c == 3 || ((mask >> c) & 1u)) return false;
    mask |= 1u << c;
  }
  return mask != 0;
}
inline bool one_context(unsigned mask) { return (mask & (mask - 1u)) == 0; }

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
// the sampled nodes' methylomes as resident handles, in the nodes' order, parsed under `contexts`
inline resident::Samples load_resident(const Inputs& in, const std::vector<std::string>* texts, unsigned contexts, bool sort,
                                       int dedup) {
  const size_t nn = in.nodes.size();
  if (texts && texts->size() != nn) throw Error(ABN_ERR_INVALID_ARG, "one text per sampled node");
  resident::Samples samples{default_device(), /*skip_lines=*/0, {}, contexts, sort, dedup};
  for (size_t i = 0; i < nn; ++i) {
    if (texts) samples.add_text((*texts)[i], in.nodes[i].file);
    else samples.add_file(in.nodes[i].file);
  }
  for (const std::string& line : samples.sort_report) diag_printf("%s", line.c_str());
  return samples;
}

// read_inputs_resident behind the loader: `in` is the graph, sites[i] node i's methylome
inline Inputs inputs_of_resident(Inputs in, const std::vector<windows::ResidentSites>& sites, double posterior_max_filter,
                                 std::vector<double>& dm, Align align) {
  std::vector<Node>& nodes = in.nodes;
  const size_t nn = nodes.size();
  Device& dev = default_device();
  std::vector<std::string> names;
  for (size_t i = 0; i < nn; ++i) names.push_back(nodes[i].file);
  Owned<abn_codes, abn_codes_destroy> codes;
  int32_t same_len = 1;
  if (nn > 0) {
    const resident::AlignMode& m = resident::align_mode(align);
    dev.check(m.codes_create(dev.get(), posterior_max_filter, (int32_t)nn, resident::pointers(sites).data(), codes.out()),
              m.codes_name);
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
    keep_transitions(in, true, [&](uint64_t* table) {
      dev.check(abn_codes_transitions(codes.get(), table), "Pedigree::build (state transitions)");
    });
    return in;
  }
  keep_transitions(in, same_len != 0, [](uint64_t*) {});  // (fewer than two samples: no pair)
  // the reference's answer for samples of different length is per pair (:221-227): the host loop gives it
  for (size_t i = 0; i < nn; ++i) {
    const windows::ResidentSites& mine = sites[i];
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

inline Inputs read_inputs_resident(const std::string& nodelist, const std::string& edgelist, double posterior_max_filter,
                                   std::vector<double>& dm, const std::vector<std::string>* texts, Align align,
                                   unsigned contexts, bool sort, int dedup) {
  Inputs in = read_graph(nodelist, edgelist);
  const resident::Samples samples = load_resident(in, texts, contexts, sort, dedup);
  return inputs_of_resident(std::move(in), samples.sites, posterior_max_filter, dm, align);
}

// Pedigree::build with --sites device once per context of a mask of SEVERAL contexts: every methylome is read and parsed
// once and split on the device; [c] = the pedigree and p0uu of context c, what build_pedigree under that context alone
// gives (an empty pedigree for a context outside the mask).
inline std::array<std::pair<Pedigree, double>, 3> build_pedigrees_by_context(const std::string& nodelist,
                                                                             const std::string& edgelist,
                                                                             double posterior_max_filter, Align align,
                                                                             unsigned contexts, bool sort = false,
                                                                             int dedup = -1) {
  const Inputs graph = read_graph(nodelist, edgelist);
  const auto by_context = load_resident(graph, nullptr, contexts, sort, dedup).split();
  std::array<std::pair<Pedigree, double>, 3> out;
  for (size_t c = 0; c < 3; ++c) {
    if (!((contexts >> c) & 1u)) continue;
    std::vector<double> dm;
    const Inputs in = inputs_of_resident(graph, by_context[c], posterior_max_filter, dm, align);
    out[c] = {convert(in, dm), in.p0uu};
  }
  return out;
}
}  // namespace detail
}  // namespace alphabeta
