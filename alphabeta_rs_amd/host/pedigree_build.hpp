// pedigree_build.hpp — Pedigree::build (src/pedigree.rs:92-337): nodelist / edgelist / methylome files ->
// (t0, t1, t2, D) rows and p0uu.  SURVEY.md §8f row 1 ("next"): host-side data preparation in front of
// the hot path, needed for the `alphabeta` CLI to be drop-in from raw inputs.  Plain C++ on the host;
// the O(pairs x sites) status comparison is integer work done once per run.
#pragma once

#include <atomic>

#include "alphabeta.hpp"
#include "transitions.hpp"

namespace alphabeta {
namespace detail {

// The diagnostics the build prints ("Warning: Encountered invalid methylation status", "Lengths do not match") go to
// stdout as they arise — or, while Pedigree::build_many reads an entry, into that entry's Built::diagnostics, so that its
// caller can print them where the per-entry loop it replaces printed them.
inline std::string*& diag_sink() {
  static thread_local std::string* sink = nullptr;
  return sink;
}
template <class... A>
inline void diag_printf(const char* fmt, A... a) {
  char buf[256];
  std::snprintf(buf, sizeof buf, fmt, a...);
  if (diag_sink()) *diag_sink() += buf;
  else std::fputs(buf, stdout);
}

struct Site {  // the fields of MethylationSite (src/methylation_site.rs:32-45) the pedigree build reads
  double posteriormax;
  uint32_t status_numeric;  // U=0, I=1, M=2 (src/methylation_site.rs:130-136)
  double meth_lvl;
};

inline std::vector<std::string> split_any(const std::string& s, const char* delims) {
  std::vector<std::string> out;
  size_t pos = 0;
  for (;;) {
    size_t e = s.find_first_of(delims, pos);
    out.push_back(s.substr(pos, e == std::string::npos ? std::string::npos : e - pos));
    if (e == std::string::npos) break;
    pos = e + 1;
  }
  return out;
}
inline bool parse_u32(const std::string& t, uint32_t& v) {  // str::parse::<u32>
  if (t.empty()) return false;
  size_t i = (t[0] == '+') ? 1 : 0;
  if (i >= t.size()) return false;
  uint64_t acc = 0;
  for (; i < t.size(); ++i) {
    if (t[i] < '0' || t[i] > '9') return false;
    acc = acc * 10 + (uint64_t)(t[i] - '0');
    if (acc > 0xffffffffull) return false;
  }
  v = (uint32_t)acc;
  return true;
}
inline bool parse_f64(const std::string& t, double& v) {  // str::parse::<f64>
  if (t.empty()) return false;
  char* e = nullptr;
  v = std::strtod(t.c_str(), &e);
  return *e == 0 && !std::isspace((unsigned char)t[0]);
}
inline bool parse_chromosome(std::string t) {  // src/methylation_site.rs:55-68
  while (t.rfind("chr", 0) == 0) t = t.substr(3);
  if (t == "M" || t == "C") return true;
  uint32_t n;
  return parse_u32(t, n) && n <= 255;
}
inline uint32_t status_from(char c) {  // src/methylation_site.rs:100-114
  if (c == 'M') return 2;
  if (c == 'I') return 1;
  if (c != 'U') diag_printf("Warning: Encountered invalid methylation status: %c. Parsed as Unmethylated\n", c);
  return 0;
}

// MethylationSite::from_methylome_file_line (src/methylation_site.rs:146-362), reduced to what
// Pedigree::build consumes.  Formats are tried in the reference's order.
inline bool parse_site(const std::string& line, Site& out) {
  const auto tab = split_any(line, "\t");
  auto cg = [&](size_t chrom, size_t s0, int s1, size_t cm, size_t ct, size_t pm, size_t st, size_t ml) -> bool {
    uint32_t u;
    double pmax, lvl;
    if (!parse_chromosome(tab[chrom]) || !parse_u32(tab[s0], u)) return false;
    if (s1 >= 0 && !parse_u32(tab[(size_t)s1], u)) return false;
    if (!parse_u32(tab[cm], u) || !parse_u32(tab[ct], u) || !parse_f64(tab[pm], pmax)) return false;
    if (tab[st].empty() || !parse_f64(tab[ml], lvl)) return false;
    out = Site{pmax, status_from(tab[st][0]), lvl};
    return true;
  };
  if (tab.size() == 9 && tab[3] == "CG" && cg(0, 1, -1, 4, 5, 6, 7, 8)) return true;    // first_format
  if (tab.size() == 10 && tab[3] == "CG" && cg(0, 1, -1, 4, 5, 6, 7, 8)) return true;   // second_format
  if (tab.size() == 11 && tab[3] == "CG" && cg(0, 1, 2, 6, 7, 8, 9, 10)) return true;   // third_format
  const auto ws = split_any(line, "\t ");
  if (ws.size() == 4) {  // chromatin-state / bigwig rows: posteriormax 0, status U, level 0
    uint32_t a, b;
    if (parse_chromosome(ws[0]) && parse_u32(ws[1], a) && parse_u32(ws[2], b)) {
      out = Site{0.0, 0, 0.0};
      return true;
    }
  }
  return false;
}

struct Node {  // src/pedigree.rs:16-26
  size_t id;
  std::string file, name;
  uint32_t generation;
  bool meth;
  double rc_meth_lvl = 0.0;
  std::vector<Site> sites;
};

inline std::string read_file(const std::string& path, const char* what) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw Error(ABN_ERR_INVALID_ARG, std::string("Error while building pedigree: could not read ") + what + " " + path);
  std::ostringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

// The first half of Pedigree::build (src/pedigree.rs:92-184): what the input files hold.
struct EdgeRef { size_t from, to; };  // indices into Inputs::all
struct Inputs {
  std::vector<Node> all;       // every row of the nodelist, :98-117
  std::vector<EdgeRef> edges;  // :124-136
  std::vector<Node> nodes;     // the sampled ("Y") nodes with their sites, :138-178
  double p0uu = 0.0;           // :180-184
  bool same_len() const {      // every sample has the sites of the first: the pairwise scan can take the code bytes
    for (size_t i = 1; i < nodes.size(); ++i)
      if (nodes[i].sites.size() != nodes[0].sites.size()) return false;
    return true;
  }
};

// the sites of a methylome text, every line read (src/pedigree.rs:147-163), parsed on the device: defined in
// windows_extract.hpp on windows::parse_sites_device
inline std::vector<Site> parse_sites_device_reduced(const std::string& text);

// the nodelist and the edgelist (src/pedigree.rs:98-136) and the sampled ("Y") nodes, their methylomes not yet read
inline Inputs read_graph(const std::string& nodelist, const std::string& edgelist) {
  Inputs in;
  const std::string nodes_txt = read_file(nodelist, "nodelist"), edges_txt = read_file(edgelist, "edgelist");
  // :98-117
  std::vector<Node>& all = in.all;
  {
    const auto lines = split_any(nodes_txt, "\n\r");
    for (size_t li = 1; li < lines.size(); ++li) {
      const auto e = split_any(lines[li], ",\t ");
      if (e.size() < 4) continue;
      uint32_t gen;
      if (!parse_u32(e[2], gen)) continue;
      all.push_back(Node{li - 1, e[0], e[1], gen, e[3] == "Y", 0.0, {}});
    }
  }
  if (all.empty()) throw Error(ABN_ERR_INVALID_ARG, "No nodes could be parsed from the nodelist");
  // :124-136
  {
    const auto lines = split_any(edges_txt, "\n\r");
    for (size_t li = 1; li < lines.size(); ++li) {
      const auto e = split_any(lines[li], "\t ,");
      if (e.size() < 2) continue;
      size_t f = all.size(), t = all.size();
      for (size_t k = 0; k < all.size(); ++k) {
        if (f == all.size() && all[k].name == e[0]) f = k;
        if (t == all.size() && all[k].name == e[1]) t = k;
      }
      if (f < all.size() && t < all.size()) in.edges.push_back(EdgeRef{f, t});
    }
  }
  for (const auto& n : all)  // :138-146
    if (n.meth) in.nodes.push_back(n);
  return in;
}

// :180-184, from the nodes' rc_meth_lvl
inline void fold_p0uu(Inputs& in) {
  double p0 = 0.0;
  for (const auto& n : in.nodes) p0 += 1.0 - n.rc_meth_lvl;
  in.p0uu = p0 / (double)in.nodes.size();
}

// device_parse: the methylome files are parsed by abn_sites_parse instead of the getline loop; the same sites.
// texts (nullable, with device_parse): the sampled nodes' methylome texts, already in memory, in the nodes' order — the
// files are not opened (scripts/codes_ab.py times the build without the file reads)
inline Inputs read_inputs(const std::string& nodelist, const std::string& edgelist, double posterior_max_filter,
                          bool device_parse = false, const std::vector<std::string>* texts = nullptr) {
  Inputs in = read_graph(nodelist, edgelist);
  // :138-178 — load the methylomes of the sampled ("Y") nodes
  std::vector<Node>& nodes = in.nodes;
  if (texts && (!device_parse || texts->size() != nodes.size()))
    throw Error(ABN_ERR_INVALID_ARG, "one text per sampled node, with device_parse");
  for (auto& node : nodes) {
    std::ifstream f;
    if (!texts) {
      f.open(node.file);
      if (!f) throw Error(ABN_ERR_INVALID_ARG, "Could not open node file: " + node.file);
    }
    if (texts) {
      node.sites = parse_sites_device_reduced((*texts)[(size_t)(&node - nodes.data())]);
    } else if (device_parse) {
      std::ostringstream ss;
      ss << f.rdbuf();
      node.sites = parse_sites_device_reduced(ss.str());
    } else {
      std::string line;
      while (std::getline(f, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        Site s;
        if (parse_site(line, s)) node.sites.push_back(s);
      }
    }
    double sum = 0.0;
    size_t cnt = 0;
    for (const auto& s : node.sites)
      if (s.posteriormax >= posterior_max_filter) {
        sum += s.meth_lvl;
        ++cnt;
      }
    node.rc_meth_lvl = sum / (double)cnt;  // :165-166
  }
  fold_p0uu(in);
  return in;
}

// The same Inputs with the sites left on the device (--sites device; defined in resident.hpp on
// windows::parse_sites_resident and abn_codes_create_parsed): every sampled node's methylome is parsed into a resident
// handle, the code matrix is packed and rc_meth_lvl folded there, and the D matrix comes from abn_codes_pairwise — no
// site reaches the host.  Samples of different length, or fewer than two: the handles are fetched into Inputs and the D
// matrix is dmatrix_on_host's, with its "Lengths do not match" lines.  dm: DMatrix::from's array.
// align: the samples are compared on the sites they share, by (chromosome, start, end, strand) — abn_codes_create_aligned,
// lifting the assumption of src/pedigree.rs:240.  The samples have the same length then, so the different-length fallback
// is never taken: the D matrix comes from the aligned handle, and rc_meth_lvl, hence p0uu, from its folds — the folds over
// the ALIGNED sites, which differ from the unaligned ones by design whenever a site was dropped.  One line per sample
// says how many sites it had and how many were kept.  Align::Union: abn_codes_create_union instead — every sample padded
// to the union of all sites with filtered placeholders, so a pair is compared on the sites both hold; rc_meth_lvl and p0uu
// keep the bits of the unaligned build (a placeholder is not counted).
// sort: every methylome is sorted by genomic position on the device behind its parse (abn_sites_sort), so files in any line
// order are aligned; one line per sample that was out of order says so.  dedup (-1: none): an ABN_DEDUP_* policy; implies the
// sort, and a sample with repeated sites is then collapsed on the device (abn_sites_dedup) and named in one more line.
inline Inputs read_inputs_resident(const std::string& nodelist, const std::string& edgelist, double posterior_max_filter,
                                   std::vector<double>& dm, const std::vector<std::string>* texts = nullptr,
                                   Align align = Align::None, unsigned contexts = 1u, bool sort = false,
                                   int dedup = -1);
// abn_codes_kernel_ms of this thread's last read_inputs_resident (merge records, merge inserted, pack, fold)
inline double* resident_kernel_ms() {
  static thread_local double ms[4] = {0.0, 0.0, 0.0, 0.0};
  return ms;
}

// one byte per (sample, site): status | 0x80 when the posterior is below the filter; sample i's sites at
// dst[i * row_stride ...] (include/abneutral.h, abn_pairwise_divergence*)
inline void write_codes(const Inputs& in, double posterior_max_filter, uint8_t* dst, size_t row_stride) {
  for (size_t i = 0; i < in.nodes.size(); ++i) {
    const auto& sites = in.nodes[i].sites;
    for (size_t k = 0; k < sites.size(); ++k)
      dst[i * row_stride + k] =
          (uint8_t)(sites[k].status_numeric | (sites[k].posteriormax < posterior_max_filter ? 0x80u : 0u));
  }
}

// the same as 2-bit fields, straight from the site records (no byte matrix in between): 0 / 1 / 2 = the status, 3 = the
// posterior is below the filter; site 16 g + 4 j + e in byte 4 g + e of the row at bits 2j..2j+1, every field from the
// last site to the end of the row 3 (include/abneutral.h, abn_pairwise_divergence_packed).  dst: nodes x row_stride bytes
inline void write_codes_packed_at(const Inputs& in, double posterior_max_filter, uint8_t* dst, size_t row_stride,
                                  size_t byte_offset);
inline void write_codes_packed(const Inputs& in, double posterior_max_filter, uint8_t* dst, size_t row_stride) {
  std::memset(dst, 0xff, in.nodes.size() * row_stride);
  write_codes_packed_at(in, posterior_max_filter, dst, row_stride, 0);
}
// ... into the columns that begin byte_offset bytes (a multiple of 4: whole dwords of 16 sites) into every row of a
// matrix whose fields are all 3 already: an entry's column range of the matrix of one Pedigree::build_many call
inline void write_codes_packed_at(const Inputs& in, double posterior_max_filter, uint8_t* dst, size_t row_stride,
                                  size_t byte_offset) {
  for (size_t i = 0; i < in.nodes.size(); ++i) {
    const auto& sites = in.nodes[i].sites;
    uint8_t* row = dst + i * row_stride + byte_offset;
    for (size_t k = 0; k < sites.size(); ++k) {
      const unsigned f = sites[k].posteriormax < posterior_max_filter ? 3u : (sites[k].status_numeric & 3u);
      row[(k >> 4) * 4 + (k & 3)] ^= (uint8_t)((3u ^ f) << (2 * ((k >> 2) & 3)));  // the field was 3
    }
  }
}
// scans Pedigree::build has sent through the packed entry (read by the tests through host_capi.cpp)
inline std::atomic<long long>& packed_scan_calls() {
  static std::atomic<long long> calls{0};
  return calls;
}

// ... builds whose codes and rc_meth_lvl folds were made on the device from resident sites (abn_codes_create_parsed)
inline std::atomic<long long>& resident_build_calls() {
  static std::atomic<long long> calls{0};
  return calls;
}

// ... and calls Pedigree::build_many has sent through abn_pairwise_divergence_windows_packed
inline std::atomic<long long>& packed_windows_scan_calls() {
  static std::atomic<long long> calls{0};
  return calls;
}

// The entries of ONE scan call of Pedigree::build_many: entries with the same number of samples, in their order, side
// by side in one packed matrix (a row per sample).  Every entry's columns start at a multiple of 256 sites (64 bytes:
// whole super-steps of the scan, whole cache-line halves) and take ceil(sites / 256) * 64 bytes of every row.
struct PackedBatch {
  size_t nn = 0;                // samples
  std::vector<size_t> members;  // the caller's entry indices
  std::vector<size_t> sites;    // of each member
  size_t stride = 0;            // bytes per row so far
  static size_t columns_bytes(size_t L) { return (L + 255) / 256 * 64; }
  // an entry of L sites still fits a call of at most cap_bytes of packed codes (an empty batch takes any entry)
  bool takes(size_t L, size_t cap_bytes) const {
    return members.empty() || nn * (stride + columns_bytes(L)) <= cap_bytes;
  }
  void add(size_t w, size_t L) {
    members.push_back(w);
    sites.push_back(L);
    stride += columns_bytes(L);
  }
};
// The batch's packed matrix and window table — what abn_pairwise_divergence_windows_packed takes — straight from the
// entries' site records: no byte matrix, no device.  entries[m] = the Inputs of member m.  Gaps between the entries and
// the rows' padding are field 3 (filtered); a batch without a site still gets one super-step per row (the scan refuses
// a null matrix).
struct PackedCall {
  std::vector<uint8_t> packed;  // [nn x stride]
  size_t stride = 0, n_sites = 0;
  std::vector<int64_t> begin, end;  // in sites, per member
};
inline PackedCall layout_packed_call(const PackedBatch& b, const std::vector<const Inputs*>& entries,
                                     double posterior_max_filter) {
  PackedCall c;
  c.stride = std::max<size_t>(b.stride, 64);
  c.n_sites = 4 * c.stride;
  c.packed.assign(b.nn * c.stride, (uint8_t)0xff);
  size_t off = 0;  // bytes into the row
  for (size_t m = 0; m < b.members.size(); ++m) {
    write_codes_packed_at(*entries[m], posterior_max_filter, c.packed.data(), c.stride, off);
    c.begin.push_back((int64_t)(4 * off));
    c.end.push_back((int64_t)(4 * off + b.sites[m]));
    off += PackedBatch::columns_bytes(b.sites[m]);
  }
  return c;
}

// DMatrix::from, :210-261 — entry [i][j - i - 1] of an nn x nn array
inline std::vector<double> dmatrix_of_pairs(size_t nn, const double* dvalue) {  // from the scan's pair order
  std::vector<double> dm(nn * nn, 0.0);
  size_t p = 0;
  for (size_t i = 0; i < nn; ++i)
    for (size_t j = i + 1; j < nn; ++j) dm[i * nn + (j - i - 1)] = dvalue[p++];
  return dm;
}
inline std::vector<double> dmatrix_on_host(const Inputs& in, double posterior_max_filter) {
  const auto& nodes = in.nodes;
  const size_t nn = nodes.size();
  std::vector<double> dm(nn * nn, 0.0);
  for (size_t i = 0; i < nn; ++i)
    for (size_t j = i + 1; j < nn; ++j) {
      const auto &a = nodes[i].sites, &b = nodes[j].sites;
      if (a.size() != b.size()) {
        diag_printf("Lengths do not match, all bets are off: %zu vs %zu\n", a.size(), b.size());
        dm[i * nn + (j - i - 1)] = 0.0;
        continue;
      }
      uint64_t div = 0, compared = 0;
      for (size_t k = 0; k < a.size(); ++k) {
        if (a[k].posteriormax < posterior_max_filter || b[k].posteriormax < posterior_max_filter) continue;
        div += a[k].status_numeric > b[k].status_numeric ? a[k].status_numeric - b[k].status_numeric
                                                         : b[k].status_numeric - a[k].status_numeric;
        ++compared;
      }
      dm[i * nn + (j - i - 1)] = (double)div / (2.0 * (double)compared);
    }
  return dm;
}

// The second half: DMatrix::convert, :263-337 — undirected graph, edge weight = |generation difference|
inline Pedigree convert(const Inputs& in, const std::vector<double>& dm) {
  const auto& all = in.all;
  const auto& edges = in.edges;
  const auto& nodes = in.nodes;
  const size_t nn = nodes.size();
  size_t vmax = 0;
  for (const auto& e : edges) vmax = std::max(vmax, std::max(all[e.from].id, all[e.to].id) + 1);
  std::vector<std::vector<std::pair<size_t, size_t>>> adj(vmax);
  for (const auto& e : edges) {
    const Node &from = all[e.from], &to = all[e.to];
    const size_t w = from.generation > to.generation ? from.generation - to.generation : to.generation - from.generation;
    adj[from.id].push_back({to.id, w});
    adj[to.id].push_back({from.id, w});
  }
  auto generation_of = [&](size_t id) -> uint32_t {  // :298-309
    for (const auto& e : edges) {
      if (all[e.from].id == id) return all[e.from].generation;
      if (all[e.to].id == id) return all[e.to].generation;
    }
    throw Error(ABN_ERR_BAD_PEDIGREE, "node on a path is not part of any edge");
  };
  Pedigree ped;
  for (size_t i = 0; i < nn; ++i)
    for (size_t j = i + 1; j < nn; ++j) {
      const size_t src = nodes[i].id, dst = nodes[j].id;
      if (src == dst || src >= vmax || dst >= vmax) continue;
      // Dijkstra (astar with a zero heuristic, :283-289)
      const size_t INF = std::numeric_limits<size_t>::max();
      std::vector<size_t> dist(vmax, INF), prev(vmax, INF);
      using QE = std::pair<size_t, size_t>;
      std::priority_queue<QE, std::vector<QE>, std::greater<QE>> pq;
      dist[src] = 0;
      pq.push({0, src});
      while (!pq.empty()) {
        auto [d, u] = pq.top();
        pq.pop();
        if (d != dist[u]) continue;
        if (u == dst) break;
        for (auto [v, w] : adj[u])
          if (d + w < dist[v]) {
            dist[v] = d + w;
            prev[v] = u;
            pq.push({dist[v], v});
          }
      }
      if (dist[dst] == INF) continue;  // None => continue, :292
      uint32_t t0 = generation_of(dst);
      for (size_t v = dst; v != src; v = prev[v]) t0 = std::min(t0, generation_of(v));
      t0 = std::min(t0, generation_of(src));
      const double t1 = (double)nodes[i].generation, t2 = (double)nodes[j].generation;
      if ((double)dist[dst] != t1 - (double)t0 + t2 - (double)t0)  // assert_eq!, :327
        throw Error(ABN_ERR_BAD_PEDIGREE, "path length does not match the generation times");
      ped.push_row((double)t0, t1, t2, dm[i * nn + (j - i - 1)]);
    }
  return ped;
}

// What convert makes of the graph alone: for every row it would emit, the pair (i, j) of sampled nodes and (t0, t1, t2).
// The windows, or tiles, of one run share one nodelist and edgelist, so the shortest-path searches run once, not once per
// window.  (convert itself on a D matrix whose entries are their own indices: the rows it emits and their order are
// convert's by construction, and so is what it throws.)
struct PairTimes {
  size_t i, j;
  double t0, t1, t2;
};
inline std::vector<PairTimes> convert_times(const Inputs& graph) {
  const size_t nn = graph.nodes.size();
  std::vector<double> where(nn * nn, 0.0);
  for (size_t i = 0; i < nn; ++i)
    for (size_t j = i + 1; j < nn; ++j) where[i * nn + (j - i - 1)] = (double)(i * nn + j);  // exact: far below 2^53
  const Pedigree p = convert(graph, where);
  std::vector<PairTimes> out;
  for (size_t r = 0; r < p.nrows(); ++r) {
    const size_t at = (size_t)p.at(r, 3);
    out.push_back(PairTimes{at / nn, at % nn, p.at(r, 0), p.at(r, 1), p.at(r, 2)});
  }
  return out;
}
// convert(graph, dm), bit for bit, from convert_times(graph); nn = graph.nodes.size()
inline Pedigree rows_from(const std::vector<PairTimes>& times, const std::vector<double>& dm, size_t nn) {
  Pedigree ped;
  for (const PairTimes& t : times) ped.push_row(t.t0, t.t1, t.t2, dm[t.i * nn + (t.j - t.i - 1)]);
  return ped;
}

// With --transitions: the table of the build's sampled nodes, appended to transitions::request().  scan(table) fills the
// [pairs x 9] counts from the code matrix the D matrix came from; samples of different length have no such matrix.
template <class Scan>
inline void keep_transitions(const Inputs& in, bool same_len, Scan scan) {
  if (!transitions::request().wanted) return;
  if (!same_len) throw Error(ABN_ERR_INVALID_ARG, "--transitions needs the same number of sites in every sample");
  transitions::Table t;
  for (const Node& n : in.nodes) {
    t.names.push_back(n.name);
    t.generations.push_back(n.generation);
  }
  t.counts.assign(t.pairs() * 9, 0);
  if (t.pairs() > 0) scan(t.counts.data());
  transitions::request().tables.push_back(std::move(t));
}

// Pedigree::build; texts: as read_inputs
inline std::pair<Pedigree, double> build_pedigree(const std::string& nodelist, const std::string& edgelist,
                                                  double posterior_max_filter, bool gpu_pairwise, bool device_parse,
                                                  bool device_sites, const std::vector<std::string>* texts = nullptr,
                                                  Align align = Align::None, unsigned contexts = 1u, bool sort = false,
                                                  int dedup = -1) {
  if (sort && !device_sites) throw Error(ABN_ERR_INVALID_ARG, "--sort needs --sites device");
  if (dedup >= 0 && !device_sites) throw Error(ABN_ERR_INVALID_ARG, "--dedup needs --sites device");
  if (align != Align::None && !device_sites)
    throw Error(ABN_ERR_INVALID_ARG, std::string("--align ") + align_name(align) + " needs --sites device");
  if (contexts != 1u && !device_sites) throw Error(ABN_ERR_INVALID_ARG, "--contexts needs --sites device");
  if (device_sites) {
    if (!device_parse || !gpu_pairwise) throw Error(ABN_ERR_INVALID_ARG, "--sites device needs --parse device");
    std::vector<double> dm;
    const Inputs in = read_inputs_resident(nodelist, edgelist, posterior_max_filter, dm, texts, align, contexts, sort, dedup);
    return {convert(in, dm), in.p0uu};
  }
  const Inputs in = read_inputs(nodelist, edgelist, posterior_max_filter, device_parse, texts);
  const size_t nn = in.nodes.size();
  std::vector<double> dm;
  if (gpu_pairwise && in.same_len() && nn >= 2) {
    const size_t L = in.nodes[0].sites.size();
    const size_t stride = (size_t)abn_packed_row_stride((int64_t)L);
    std::vector<uint8_t> packed(nn * stride);  // a quarter of the code bytes to hold and to upload
    write_codes_packed(in, posterior_max_filter, packed.data(), stride);
    std::vector<double> dv(nn * (nn - 1) / 2);
    Device& dev = default_device();
    dev.check(abn_pairwise_divergence_packed(dev.get(), packed.data(), (int32_t)nn, (int64_t)L, (int64_t)stride, nullptr,
                                             nullptr, dv.data()),
              "Pedigree::build (pairwise divergence)");
    packed_scan_calls().fetch_add(1, std::memory_order_relaxed);
    dm = dmatrix_of_pairs(nn, dv.data());
    keep_transitions(in, true, [&](uint64_t* table) {
      dev.check(abn_pairwise_transitions_packed(dev.get(), packed.data(), (int32_t)nn, (int64_t)L, (int64_t)stride, table),
                "Pedigree::build (state transitions)");
    });
  } else {
    dm = dmatrix_on_host(in, posterior_max_filter);
    keep_transitions(in, in.same_len(), [](uint64_t*) {});  // (fewer than two samples: no pair)
  }
  return {convert(in, dm), in.p0uu};
}
}  // namespace detail

inline std::pair<Pedigree, double> Pedigree::build(const std::string& nodelist, const std::string& edgelist,
                                                   double posterior_max_filter, bool gpu_pairwise,
                                                   bool device_parse, bool device_sites, Align align, unsigned contexts,
                                                   bool sort, int dedup) {
  return detail::build_pedigree(nodelist, edgelist, posterior_max_filter, gpu_pairwise, device_parse, device_sites, nullptr,
                                align, contexts, sort, dedup);
}

// Pedigree::build for many (nodelist, edgelist) pairs — the windows of src/cli/metaprofile.rs:50-72.  With gpu_pairwise
// the entries whose samples all have the same number of sites are batched by sample count: each batch's entries are
// packed straight from their site records into one 2-bit matrix (layout_packed_call: a row per sample, an entry's sites
// a column range) and scanned by ONE abn_pairwise_divergence_windows_packed call; the rest (and everything without
// gpu_pairwise) takes the host loop as build does.  An entry that fails keeps its error text and never stops the others.
// A batch is scanned when the next entry would take its matrix beyond kBuildManyCodeBytes of packed codes, all open
// batches when the site records they wait with (24 bytes per site and sample, against a quarter of a byte packed) pass
// kBuildManySiteBytes, and what is left at the end; entries are never reordered.  Host memory: those site records, one
// call's packed matrix, and the graphs.
inline std::vector<Pedigree::Built> Pedigree::build_many(const std::vector<std::pair<std::string, std::string>>& lists,
                                                         double posterior_max_filter, bool gpu_pairwise,
                                                         bool device_parse) {
  using namespace detail;
  const size_t W = lists.size();
  std::vector<Built> out(W);
  std::vector<Inputs> in(W);
  std::vector<std::vector<double>> dm(W);
  std::vector<char> alive(W, 0);
  auto fail = [&](size_t w, const std::exception& e) {
    out[w].error = e.what();
    alive[w] = 0;
  };
  // What stays of an entry until the end is its graph (names, ids, generations, edges) and its D matrix; the site records
  // are dropped as soon as the D matrix (host loop) or the entry's columns of a call's matrix (scan) are written.
  auto drop_sites = [&](size_t w) {
    for (auto& node : in[w].nodes) std::vector<Site>().swap(node.sites);
  };
  std::map<size_t, PackedBatch> open;  // sample count -> the entries waiting for their scan, in order
  size_t waiting_site_bytes = 0;
  auto scan = [&](PackedBatch& b) {
    if (b.members.empty()) return;
    const size_t nn = b.nn, npairs = nn * (nn - 1) / 2, M = b.members.size();
    try {
      std::vector<const Inputs*> entries;
      for (size_t w : b.members) entries.push_back(&in[w]);
      const PackedCall c = layout_packed_call(b, entries, posterior_max_filter);
      for (size_t w : b.members) drop_sites(w);
      std::vector<double> dv(M * npairs);
      Device& dev = default_device();
      dev.check(abn_pairwise_divergence_windows_packed(dev.get(), c.packed.data(), (int32_t)nn, (int64_t)c.n_sites,
                                                       (int64_t)c.stride, c.begin.data(), c.end.data(), (int32_t)M,
                                                       nullptr, nullptr, dv.data()),
                "Pedigree::build (pairwise divergence)");
      packed_windows_scan_calls().fetch_add(1, std::memory_order_relaxed);
      for (size_t m = 0; m < M; ++m) dm[b.members[m]] = dmatrix_of_pairs(nn, dv.data() + m * npairs);
    } catch (const std::exception& e) {
      for (size_t w : b.members) {
        drop_sites(w);
        fail(w, e);
      }
    }
    for (size_t L : b.sites) waiting_site_bytes -= nn * L * sizeof(Site);
    const size_t nn_keep = b.nn;
    b = PackedBatch{};
    b.nn = nn_keep;
  };
  for (size_t w = 0; w < W; ++w) {
    diag_sink() = &out[w].diagnostics;
    bool waits = false;
    try {
      in[w] = read_inputs(lists[w].first, lists[w].second, posterior_max_filter, device_parse);
      alive[w] = 1;
      const size_t nn = in[w].nodes.size();
      if (gpu_pairwise && in[w].same_len() && nn >= 2) {
        waits = true;
      } else {
        dm[w] = dmatrix_on_host(in[w], posterior_max_filter);
      }
    } catch (const std::exception& e) {
      fail(w, e);
    }
    diag_sink() = nullptr;
    if (!waits) {
      drop_sites(w);
      continue;
    }
    const size_t nn = in[w].nodes.size(), L = in[w].nodes[0].sites.size();
    PackedBatch& b = open[nn];
    b.nn = nn;
    if (!b.takes(L, kBuildManyCodeBytes)) scan(b);
    b.add(w, L);
    waiting_site_bytes += nn * L * sizeof(Site);
    if (waiting_site_bytes > kBuildManySiteBytes)
      for (auto& kv : open) scan(kv.second);
  }
  for (auto& kv : open) scan(kv.second);
  for (size_t w = 0; w < W; ++w) {
    if (!alive[w]) continue;
    try {
      out[w].pedigree = convert(in[w], dm[w]);
      out[w].p0uu = in[w].p0uu;
      out[w].ok = true;
    } catch (const std::exception& e) {
      fail(w, e);
    }
  }
  return out;
}

}  // namespace alphabeta
