// windows_extract.hpp — the host half of the reference's `extract` stage (src/extract.rs:17-155): the annotation parser
// (src/genes.rs:140-217), the full methylome-line parse (src/methylation_site.rs:146-362) and the choice of a gene for
// every site (src/windows.rs:303-338 around is_in_gene / find_gene, src/methylation_site.rs:368-418).  What follows the
// gene choice — place_in_windows, the per-window site lists, the packed matrix, the folds — runs on the device
// (abn_windows_*, csrc/abn_windows.hpp).  The gene choice (the last_gene cache: a few integer compares per site, each
// depending on the site before) runs here, one methylome per thread (choose_genes), or on the device, where the
// dependence is resolved per block of sites (abn_genes_*, csrc/abn_genes.hpp; the Handle made from FullSite vectors):
// the same arrays either way.  Integer arithmetic wraps as the reference's release build does.  The line parse also runs
// on the device (parse_sites_device over abn_sites_parse, csrc/abn_parse.hpp): the same FullSite sequence, fed to either
// gene choice.  parse_sites_resident leaves that sequence on the device instead (abn_sites_parse_dev, abn_sites_insert),
// for the Handle made from ResidentSites (abn_windows_create_parsed); what is built from those handles — the three
// align modes, their report, the pedigree build of `alphabeta --sites device` — is resident.hpp, included at the end.
#pragma once

#include <thread>

#include "alphabeta.hpp"

namespace alphabeta {
namespace windows {

enum Strand : uint8_t { Sense = 0, Antisense = 1, Unknown = 2 };  // src/genes.rs:13-18
// Strand::eq (src/genes.rs:88-96): Unknown equals both
inline bool strand_eq(Strand a, Strand b) { return !((a == Sense && b == Antisense) || (a == Antisense && b == Sense)); }

// Chromosome (src/methylation_site.rs:48-68) as one integer: Numbered(n) = n, Mitochondrial = 256, Chloroplast = 257
inline bool parse_chromosome_key(std::string t, int& key) {
  while (t.rfind("chr", 0) == 0) t = t.substr(3);
  if (t == "M") return key = 256, true;
  if (t == "C") return key = 257, true;
  uint32_t n;
  if (!detail::parse_u32(t, n) || n > 255) return false;
  return key = (int)n, true;
}

struct Gene {  // src/genes.rs:117-125 (the annotation column is not kept)
  int chromosome;
  uint32_t start, end;
  Strand strand;
  std::string name;
};

// Gene::from_annotation_file_line, src/genes.rs:166-216 (without --invert).  Six fields split at ' ' and '\t'; the first
// format has the strand last, the second (seqnames start end width strand id) has it fifth; a line whose strand is in
// the right place but whose numbers do not parse is dropped, not handed to the other format (:203).
inline bool parse_gene_line(const std::string& line, Gene& out) {
  const auto f = detail::split_any(line, " \t");
  if (f.size() != 6) return false;
  auto correct = [](const std::string& s) { return s == "+" || s == "-" || s == "*"; };
  auto strand_of = [](const std::string& s) { return s == "+" ? Sense : (s == "-" ? Antisense : Unknown); };
  size_t strand, name;
  if (correct(f[5])) strand = 5, name = 3;
  else if (correct(f[4])) strand = 4, name = 5;
  else return false;
  Gene g;
  if (!parse_chromosome_key(f[0], g.chromosome) || !detail::parse_u32(f[1], g.start) || !detail::parse_u32(f[2], g.end))
    return false;
  g.strand = strand_of(f[strand]);
  g.name = f[name];
  out = std::move(g);
  return true;
}

struct GenesByStrand {  // src/genes.rs:127-163
  std::vector<Gene> sense, antisense, combined;
};
struct Genome {
  std::map<int, GenesByStrand> chromosomes;
  size_t n_genes = 0;
  uint32_t max_gene_length = 0;  // max(end - start), src/extract.rs:53-57
};

inline std::vector<std::string> lines_of(const std::string& text) {  // BufRead::lines: "\n" or "\r\n" ends a line
  std::vector<std::string> lines = detail::split_any(text, "\n");
  if (!lines.empty() && lines.back().empty()) lines.pop_back();
  for (auto& l : lines)
    if (!l.empty() && l.back() == '\r') l.pop_back();
  return lines;
}

// src/extract.rs:30-67: every line that parses, by chromosome, each list sorted by start with a STABLE sort
inline Genome parse_annotation(const std::string& text) {
  Genome g;
  for (const auto& line : lines_of(text)) {
    Gene gene;
    if (!parse_gene_line(line, gene)) continue;
    g.max_gene_length = std::max(g.max_gene_length, gene.end - gene.start);
    ++g.n_genes;
    GenesByStrand& c = g.chromosomes[gene.chromosome];
    c.combined.push_back(gene);
    if (gene.strand == Sense) c.sense.push_back(gene);
    else if (gene.strand == Antisense) c.antisense.push_back(gene);
  }
  auto by_start = [](const Gene& a, const Gene& b) { return a.start < b.start; };
  for (auto& kv : g.chromosomes) {
    std::stable_sort(kv.second.sense.begin(), kv.second.sense.end(), by_start);
    std::stable_sort(kv.second.antisense.begin(), kv.second.antisense.end(), by_start);
    std::stable_sort(kv.second.combined.begin(), kv.second.combined.end(), by_start);
  }
  return g;
}

struct FullSite {  // the fields of MethylationSite (src/methylation_site.rs:32-45) the extraction reads
  int chromosome;
  uint32_t start, end;
  Strand strand;
  double posteriormax;
  uint32_t status_numeric;
  double meth_lvl;
  uint8_t context;  // 0 CG, 1 CHG, 2 CHH; 3: a row without a context field
};

// field 3 of the 9-, 10- and 11-field formats -> its context code when the mask `contexts` (1 CG, 2 CHG, 4 CHH) holds
// it, else -1: the line is no site
inline int context_in_mask(const std::string& field, unsigned contexts) {
  const int code = field == "CG" ? 0 : (field == "CHG" ? 1 : (field == "CHH" ? 2 : -1));
  return code >= 0 && ((contexts >> code) & 1u) ? code : -1;
}

// MethylationSite::from_methylome_file_line (src/methylation_site.rs:146-362, without --invert): detail::parse_site with
// the coordinates kept.  A single location gets end = start + 1; the 4-field rows (chromatin state, bigwig) have an
// Unknown strand, posterior 0, status U, level 0, and no context: every mask accepts them.  contexts: the mask of the
// contexts whose lines are sites; the reference reads CG alone (:150,193), the default.
inline bool parse_site_full(const std::string& line, FullSite& out, unsigned contexts = 1u) {
  const auto tab = detail::split_any(line, "\t");
  const int ctx = tab.size() >= 9 && tab.size() <= 11 ? context_in_mask(tab[3], contexts) : -1;
  auto cg = [&](size_t chrom, size_t s0, int s1, size_t strand, size_t cm, size_t ct, size_t pm, size_t st, size_t ml) {
    FullSite s;
    uint32_t u;
    if (!parse_chromosome_key(tab[chrom], s.chromosome) || !detail::parse_u32(tab[s0], s.start)) return false;
    s.end = s.start + 1u;
    if (s1 >= 0 && !detail::parse_u32(tab[(size_t)s1], s.end)) return false;
    if (!detail::parse_u32(tab[cm], u) || !detail::parse_u32(tab[ct], u) || !detail::parse_f64(tab[pm], s.posteriormax))
      return false;
    if (tab[st].empty() || !detail::parse_f64(tab[ml], s.meth_lvl)) return false;
    s.strand = tab[strand] == "+" ? Sense : Antisense;
    s.status_numeric = detail::status_from(tab[st][0]);
    s.context = (uint8_t)ctx;
    out = s;
    return true;
  };
  if (tab.size() == 9 && ctx >= 0 && cg(0, 1, -1, 2, 4, 5, 6, 7, 8)) return true;    // first_format
  if (tab.size() == 10 && ctx >= 0 && cg(0, 1, -1, 2, 4, 5, 6, 7, 8)) return true;   // second_format
  if (tab.size() == 11 && ctx >= 0 && cg(0, 1, 2, 5, 6, 7, 8, 9, 10)) return true;   // third_format
  const auto ws = detail::split_any(line, "\t ");
  if (ws.size() == 4) {
    FullSite s{0, 0, 0, Unknown, 0.0, 0, 0.0, 3};
    if (parse_chromosome_key(ws[0], s.chromosome) && detail::parse_u32(ws[1], s.start) && detail::parse_u32(ws[2], s.end)) {
      out = s;
      return true;
    }
  }
  return false;
}

// The sites of a methylome text in file order — the lines from skip_lines on that from_methylome_file_line accepts
// (src/windows.rs:303-306 skips the header row, src/pedigree.rs:147-163 skips nothing) — parsed on the host.
// line_numbers (nullable): every site's line, counted from 0 in the text.
inline std::vector<FullSite> parse_sites_host(const std::string& text, size_t skip_lines = 1,
                                              std::vector<int64_t>* line_numbers = nullptr, unsigned contexts = 1u) {
  std::vector<FullSite> out;
  const auto lines = lines_of(text);
  for (size_t li = skip_lines; li < lines.size(); ++li) {
    FullSite s;
    if (!parse_site_full(lines[li], s, contexts)) continue;
    out.push_back(s);
    if (line_numbers) line_numbers->push_back((int64_t)li);
  }
  return out;
}

// ... parsed on the device (abn_sites_parse): exactly the sequence parse_sites_host yields.  The records the device
// accepted are merged by line number with the lines it deferred (an f64 field it cannot be certain of, a line beyond its
// staging limit), each decided here by parse_site_full; the invalid-status warnings are printed in file order.
inline std::vector<FullSite> parse_sites_device(Device& dev, const std::string& text, size_t skip_lines = 1,
                                                int64_t slab_bytes = 0, std::vector<int64_t>* line_numbers = nullptr) {
  abn_sites_params p{};
  p.slab_bytes = slab_bytes;
  p.skip_lines = (int32_t)skip_lines;
  abn_sites* h = nullptr;
  dev.check(abn_sites_parse(dev.get(), text.data(), (int64_t)text.size(), &p, &h), "abn_sites_parse");
  const Owned<abn_sites, abn_sites_destroy> guard(h);
  int64_t n = 0, nd = 0;
  abn_sites_info(h, &n, &nd, nullptr, nullptr);
  std::vector<int64_t> line((size_t)n), dline((size_t)nd), doff((size_t)nd), dlen((size_t)nd);
  std::vector<int32_t> chrom((size_t)n);
  std::vector<uint32_t> start((size_t)n), end((size_t)n);
  std::vector<uint8_t> strand((size_t)n), status((size_t)n), flag((size_t)n);
  std::vector<double> pm((size_t)n), ml((size_t)n);
  abn_sites_fetch(h, line.data(), chrom.data(), start.data(), end.data(), strand.data(), pm.data(), status.data(),
                  flag.data(), ml.data());
  abn_sites_deferred(h, dline.data(), doff.data(), dlen.data());
  // a flagged record's warning names the status byte: that line is read again here, through an index of the text's line
  // begins made when the first such record turns up
  std::vector<size_t> begins;
  auto warn = [&](int64_t l) {
    if (begins.empty()) {
      begins.push_back(0);
      for (const char* q = text.data(); (q = (const char*)std::memchr(q, '\n', (size_t)(text.data() + text.size() - q)));)
        begins.push_back((size_t)(++q - text.data()));
    }
    const size_t b = begins[(size_t)l], e = (size_t)l + 1 < begins.size() ? begins[(size_t)l + 1] - 1 : text.size();
    std::string s = text.substr(b, e - b);
    if (!s.empty() && s.back() == '\r') s.pop_back();
    FullSite again;
    parse_site_full(s, again);
  };
  std::vector<FullSite> out;
  out.reserve((size_t)n);
  size_t i = 0, j = 0;
  while (i < (size_t)n || j < (size_t)nd) {
    if (j == (size_t)nd || (i < (size_t)n && line[i] < dline[j])) {
      if (flag[i]) warn(line[i]);
      out.push_back(FullSite{chrom[i], start[i], end[i], (Strand)strand[i], pm[i], status[i], ml[i]});
      if (line_numbers) line_numbers->push_back(line[i]);
      ++i;
    } else {
      FullSite s;
      if (parse_site_full(text.substr((size_t)doff[j], (size_t)dlen[j]), s)) {
        out.push_back(s);
        if (line_numbers) line_numbers->push_back(dline[j]);
      }
      ++j;
    }
  }
  return out;
}

// abn_sites in its resident form: one methylome's records on the device, its deferred lines decided and inserted
struct ResidentSites : Owned<abn_sites, abn_sites_destroy> {
  using Owned::Owned;
  size_t size() const {  // the sites of the merged sequence
    int64_t n = 0;
    abn_sites_info(get(), &n, nullptr, nullptr, nullptr);
    return (size_t)n;
  }
};

// ... parsed on the device and LEFT there (abn_sites_parse_dev): the sequence parse_sites_device yields, as a handle.
// Only the deferred triples and the flagged records' lines come back; every deferred line is decided here by
// parse_site_full and the accepted ones go back up (abn_sites_insert).  The invalid-status warnings of the flagged
// records and of the deferred lines are printed in one walk in file order, as parse_sites_device prints them.
inline ResidentSites parse_sites_resident(Device& dev, const std::string& text, size_t skip_lines = 1,
                                          int64_t slab_bytes = 0, unsigned contexts = 1u) {
  abn_sites_params p{};
  p.slab_bytes = slab_bytes;
  p.skip_lines = (int32_t)skip_lines;
  p.contexts = contexts == 1u ? 0 : (int32_t)contexts;
  abn_sites* h = nullptr;
  dev.check(abn_sites_parse_dev(dev.get(), text.data(), (int64_t)text.size(), &p, &h), "abn_sites_parse_dev");
  ResidentSites out(h);
  int64_t nd = 0, nf = 0;
  abn_sites_info(h, nullptr, &nd, nullptr, nullptr);
  abn_sites_flagged(h, &nf, nullptr);
  std::vector<int64_t> flagged((size_t)nf), dline((size_t)nd), doff((size_t)nd), dlen((size_t)nd);
  abn_sites_flagged(h, nullptr, flagged.data());
  abn_sites_deferred(h, dline.data(), doff.data(), dlen.data());
  std::vector<size_t> begins;  // the text's line begins, indexed when the first flagged record turns up
  auto warn = [&](int64_t l) {
    if (begins.empty()) {
      begins.push_back(0);
      for (const char* q = text.data(); (q = (const char*)std::memchr(q, '\n', (size_t)(text.data() + text.size() - q)));)
        begins.push_back((size_t)(++q - text.data()));
    }
    const size_t b = begins[(size_t)l], e = (size_t)l + 1 < begins.size() ? begins[(size_t)l + 1] - 1 : text.size();
    std::string s = text.substr(b, e - b);
    if (!s.empty() && s.back() == '\r') s.pop_back();
    FullSite again;
    parse_site_full(s, again, contexts);
  };
  std::vector<int64_t> line;
  std::vector<int32_t> chrom;
  std::vector<uint32_t> start, end;
  std::vector<uint8_t> strand, status, context;
  std::vector<double> pm, ml;
  size_t i = 0, j = 0;
  while (i < flagged.size() || j < dline.size()) {
    if (j == dline.size() || (i < flagged.size() && flagged[i] < dline[j])) {
      warn(flagged[i++]);
      continue;
    }
    FullSite s;
    if (parse_site_full(text.substr((size_t)doff[j], (size_t)dlen[j]), s, contexts)) {
      line.push_back(dline[j]);
      chrom.push_back(s.chromosome);
      start.push_back(s.start);
      end.push_back(s.end);
      strand.push_back((uint8_t)s.strand);
      pm.push_back(s.posteriormax);
      status.push_back((uint8_t)s.status_numeric);
      ml.push_back(s.meth_lvl);
      context.push_back(s.context);
    }
    ++j;
  }
  dev.check(abn_sites_insert_ctx(h, (int64_t)line.size(), line.data(), chrom.data(), start.data(), end.data(),
                                 strand.data(), pm.data(), status.data(), ml.data(), context.data()),
            "abn_sites_insert_ctx");
  return out;
}

struct GeneRule {  // the two arguments is_in_gene and find_gene read
  uint32_t cutoff = 2048;
  bool cutoff_gene_length = false;
};

// src/methylation_site.rs:368-378
inline bool is_in_gene(const FullSite& s, const Gene& g, const GeneRule& r) {
  const uint32_t cutoff = r.cutoff_gene_length ? g.end - g.start : r.cutoff;
  return s.chromosome == g.chromosome && g.start <= s.start + cutoff && s.end <= g.end + cutoff &&
         strand_eq(s.strand, g.strand);
}

// src/methylation_site.rs:385-418.  The lists are sorted by start while the search key is end + cutoff, so with nested or
// equal-keyed genes the answer depends on the probe sequence: this is slice::binary_search_by of the standard library
// (the `size / 2` form of Rust 1.52 to 1.81), probe for probe.
inline const Gene* find_gene(const FullSite& s, const Genome& genome, const GeneRule& r) {
  const auto it = genome.chromosomes.find(s.chromosome);
  if (it == genome.chromosomes.end()) return nullptr;
  const std::vector<Gene>& list =
      s.strand == Sense ? it->second.sense : (s.strand == Antisense ? it->second.antisense : it->second.combined);
  auto key = [&](const Gene& g) { return r.cutoff_gene_length ? g.end + (g.end - g.start) : g.end + r.cutoff; };
  size_t size = list.size(), left = 0, right = size, found = size;
  bool exact = false;
  while (left < right) {
    const size_t mid = left + size / 2;
    const uint32_t k = key(list[mid]);
    if (k == s.start) {
      found = mid;
      exact = true;
      break;
    }
    if (k < s.start) left = mid + 1;
    else right = mid;
    size = right - left;
  }
  if (!exact) found = left;
  if (found >= list.size()) return nullptr;
  return is_in_gene(s, list[found], r) ? &list[found] : nullptr;
}

// One methylome in the arrays abn_windows_create takes (a sample's slice of them).
struct SampleSites {
  std::vector<uint32_t> pos, gene_start, gene_end;
  std::vector<uint8_t> flags, code;
  std::vector<double> level;
  size_t size() const { return pos.size(); }
};

// One step of the loop of Windows::extract (src/windows.rs:325-338) up to the call of place_in_windows: a site keeps the
// previous site's gene while is_in_gene holds.
inline void choose_gene(const FullSite& s, const Gene*& last, const Genome& genome, const GeneRule& rule,
                        double posterior_max_filter, SampleSites& out) {
  if (!last || !is_in_gene(s, *last, rule)) last = find_gene(s, genome, rule);
  out.pos.push_back(s.start);
  out.gene_start.push_back(last ? last->start : 0);
  out.gene_end.push_back(last ? last->end : 0);
  out.flags.push_back((uint8_t)((s.strand == Antisense ? 1u : 0u) | (last ? 2u : 0u)));
  out.code.push_back((uint8_t)(s.status_numeric | (s.posteriormax < posterior_max_filter ? 0x80u : 0u)));
  out.level.push_back(s.meth_lvl);
}

// The loop of Windows::extract (src/windows.rs:303-338) up to the call of place_in_windows: the header row is skipped
// (`lines.skip(1)`), a line that is no site is passed over.
inline SampleSites choose_genes(const std::string& methylome_text, const Genome& genome, const GeneRule& rule,
                                double posterior_max_filter) {
  SampleSites out;
  const Gene* last = nullptr;
  const auto lines = lines_of(methylome_text);
  for (size_t li = 1; li < lines.size(); ++li) {
    FullSite s;
    if (!parse_site_full(lines[li], s)) continue;
    choose_gene(s, last, genome, rule, posterior_max_filter, out);
  }
  return out;
}
// ... on the sites already parsed (parse_sites_device, parse_sites_host), in file order
inline SampleSites choose_genes(const std::vector<FullSite>& sites, const Genome& genome, const GeneRule& rule,
                                double posterior_max_filter) {
  SampleSites out;
  const Gene* last = nullptr;
  for (const FullSite& s : sites) choose_gene(s, last, genome, rule, posterior_max_filter, out);
  return out;
}

// Windows::new (src/windows.rs:28-44): floor(max / step) windows per region, in the order upstream, gene, downstream
inline abn_windows_params window_params(uint32_t cutoff, uint32_t step, uint32_t size, bool absolute,
                                        uint32_t max_gene_length) {
  abn_windows_params p{};
  p.cutoff = cutoff;
  p.step = step;
  p.size = size;
  p.absolute = absolute ? 1 : 0;
  p.n_upstream = p.n_downstream = (int32_t)((absolute ? cutoff : 100u) / step);
  p.n_gene = (int32_t)((absolute ? max_gene_length : 100u) / step);
  return p;
}

// choose_genes for every methylome text, one per thread (at most max_threads at a time), in the order given
inline std::vector<SampleSites> choose_genes_many(const std::vector<std::string>& texts, const Genome& genome,
                                                  const GeneRule& rule, double posterior_max_filter,
                                                  size_t max_threads = 16) {
  std::vector<SampleSites> out(texts.size());
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t i; (i = next.fetch_add(1)) < texts.size();) out[i] = choose_genes(texts[i], genome, rule, posterior_max_filter);
  };
  const size_t nt = std::max<size_t>(1, std::min(max_threads, texts.size()));
  std::vector<std::thread> pool;
  for (size_t t = 1; t < nt; ++t) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
  return out;
}

// ... with the texts parsed on the device, one after the other on the calling thread (a context serves one call at a
// time); every text's gene choice runs on a thread of its own while the next text is parsed
inline std::vector<SampleSites> choose_genes_many_device(Device& dev, const std::vector<std::string>& texts,
                                                         const Genome& genome, const GeneRule& rule,
                                                         double posterior_max_filter) {
  std::vector<SampleSites> out(texts.size());
  std::vector<std::vector<FullSite>> sites(texts.size());
  std::vector<std::thread> pool;
  struct Join {
    std::vector<std::thread>& pool;
    ~Join() {
      for (auto& t : pool) t.join();
    }
  } join{pool};
  for (size_t i = 0; i < texts.size(); ++i) {
    sites[i] = parse_sites_device(dev, texts[i]);
    pool.emplace_back([&, i]() {
      out[i] = choose_genes(sites[i], genome, rule, posterior_max_filter);
      std::vector<FullSite>().swap(sites[i]);
    });
  }
  return out;
}

// The sites of every methylome text in the order given (parse_sites_host on at most max_threads threads, or
// parse_sites_device one text after the other: a context serves one call at a time)
inline std::vector<std::vector<FullSite>> parse_sites_many(const std::vector<std::string>& texts, Device* dev,
                                                           size_t max_threads = 16) {
  std::vector<std::vector<FullSite>> out(texts.size());
  if (dev) {
    for (size_t i = 0; i < texts.size(); ++i) out[i] = parse_sites_device(*dev, texts[i]);
    return out;
  }
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t i; (i = next.fetch_add(1)) < texts.size();) out[i] = parse_sites_host(texts[i]);
  };
  const size_t nt = std::max<size_t>(1, std::min(max_threads, texts.size()));
  std::vector<std::thread> pool;
  for (size_t t = 1; t < nt; ++t) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
  return out;
}

// choose_genes for every sample's parsed sites, one per thread (at most max_threads at a time)
inline std::vector<SampleSites> choose_genes_many(const std::vector<std::vector<FullSite>>& sites, const Genome& genome,
                                                  const GeneRule& rule, double posterior_max_filter,
                                                  size_t max_threads = 16) {
  std::vector<SampleSites> out(sites.size());
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t i; (i = next.fetch_add(1)) < sites.size();) out[i] = choose_genes(sites[i], genome, rule, posterior_max_filter);
  };
  const size_t nt = std::max<size_t>(1, std::min(max_threads, sites.size()));
  std::vector<std::thread> pool;
  for (size_t t = 1; t < nt; ++t) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
  return out;
}

// The Genome in the arrays abn_genes_create takes: every non-empty list of every chromosome (kind 0 sense, 1 antisense,
// 2 combined), in the order parse_annotation left it — sorted by start, stably
struct GeneLists {
  std::vector<int32_t> list_chromosome, list_kind;
  std::vector<int64_t> list_offset{0};
  std::vector<uint32_t> start, end;
  std::vector<uint8_t> strand;
};
inline GeneLists flatten_genome(const Genome& genome) {
  GeneLists out;
  for (const auto& kv : genome.chromosomes) {
    const std::vector<Gene>* lists[3] = {&kv.second.sense, &kv.second.antisense, &kv.second.combined};
    for (int kind = 0; kind < 3; ++kind) {
      if (lists[kind]->empty()) continue;
      out.list_chromosome.push_back(kv.first);
      out.list_kind.push_back(kind);
      for (const Gene& g : *lists[kind]) {
        out.start.push_back(g.start);
        out.end.push_back(g.end);
        out.strand.push_back((uint8_t)g.strand);
      }
      out.list_offset.push_back((int64_t)out.start.size());
    }
  }
  return out;
}

// The samples' sites in the arrays abn_genes_choose and abn_windows_create_sites take; code = status | 0x80 when the
// posterior is below the filter, as choose_gene computes it
struct SiteArrays {
  std::vector<int64_t> offset;
  std::vector<int32_t> chromosome;
  std::vector<uint32_t> start, end;
  std::vector<uint8_t> strand, code;
  std::vector<double> level;
};
inline SiteArrays site_arrays(const std::vector<std::vector<FullSite>>& samples, double posterior_max_filter) {
  SiteArrays a;
  a.offset.assign(samples.size() + 1, 0);
  for (size_t s = 0; s < samples.size(); ++s) a.offset[s + 1] = a.offset[s] + (int64_t)samples[s].size();
  const size_t S = (size_t)a.offset.back();
  a.chromosome.resize(S);
  a.start.resize(S);
  a.end.resize(S);
  a.strand.resize(S);
  a.code.resize(S);
  a.level.resize(S);
  size_t i = 0;
  for (const auto& sample : samples)
    for (const FullSite& s : sample) {
      a.chromosome[i] = s.chromosome;
      a.start[i] = s.start;
      a.end[i] = s.end;
      a.strand[i] = (uint8_t)s.strand;
      a.code[i] = (uint8_t)(s.status_numeric | (s.posteriormax < posterior_max_filter ? 0x80u : 0u));
      a.level[i] = s.meth_lvl;
      ++i;
    }
  return a;
}

// abn_genes over a Genome
struct GenesHandle : Owned<abn_genes, abn_genes_destroy> {
  GenesHandle(Device& dev, const Genome& genome) {
    const GeneLists l = flatten_genome(genome);
    dev.check(abn_genes_create(dev.get(), (int32_t)l.list_kind.size(), l.list_chromosome.data(), l.list_kind.data(),
                               l.list_offset.data(), l.start.data(), l.end.data(), l.strand.data(), out()),
              "abn_genes_create");
  }
};

// RAII abn_windows over the samples' concatenated arrays
class Handle {
 public:
  // ... from the parsed sites: the gene of every site chosen on the device, nothing coming back before the windows are
  // placed (abn_windows_create_sites)
  Handle(Device& dev, const abn_windows_params& p, const Genome& genome, const GeneRule& rule, double posterior_max_filter,
         const std::vector<std::vector<FullSite>>& samples)
      : n_(samples.size()) {
    const GenesHandle genes(dev, genome);
    const SiteArrays a = site_arrays(samples, posterior_max_filter);
    const abn_gene_rule r{rule.cutoff, rule.cutoff_gene_length ? 1 : 0};
    dev.check(abn_windows_create_sites(dev.get(), &p, genes.get(), &r, (int32_t)n_, a.offset.data(), a.chromosome.data(),
                                       a.start.data(), a.end.data(), a.strand.data(), a.code.data(), a.level.data(), h_.out()),
              "abn_windows_create_sites");
    fetch();
  }
  // ... from the resident parse results (parse_sites_resident): merged, chosen and placed on the device, no site record
  // coming back (abn_windows_create_parsed).  align: only the sites every sample shares, by (chromosome, start, end,
  // strand), are placed (abn_windows_create_aligned): no window is ragged, and count, kept and the level sums — hence the
  // side files and every window's p0uu — describe the ALIGNED sites, not each file's own.  Align::Union: every sample gets
  // all the sites any sample holds, filtered placeholders where it lacks one (abn_windows_create_union): no window is
  // ragged, count counts union sites, kept and level_sum_kept stay each file's own.  What the alignment made of the
  // samples: resident::align_counts.  Defined in resident.hpp, on its table of the three create calls.
  Handle(Device& dev, const abn_windows_params& p, const Genome& genome, const GeneRule& rule, double posterior_max_filter,
         const std::vector<ResidentSites>& samples, Align align = Align::None);
  Handle(Device& dev, const abn_windows_params& p, const std::vector<SampleSites>& samples) : n_(samples.size()) {
    std::vector<int64_t> off(n_ + 1, 0);
    for (size_t s = 0; s < n_; ++s) off[s + 1] = off[s] + (int64_t)samples[s].size();
    SampleSites all;
    for (const auto& s : samples) {
      all.pos.insert(all.pos.end(), s.pos.begin(), s.pos.end());
      all.gene_start.insert(all.gene_start.end(), s.gene_start.begin(), s.gene_start.end());
      all.gene_end.insert(all.gene_end.end(), s.gene_end.begin(), s.gene_end.end());
      all.flags.insert(all.flags.end(), s.flags.begin(), s.flags.end());
      all.code.insert(all.code.end(), s.code.begin(), s.code.end());
      all.level.insert(all.level.end(), s.level.begin(), s.level.end());
    }
    dev.check(abn_windows_create(dev.get(), &p, (int32_t)n_, off.data(), all.pos.data(), all.gene_start.data(),
                                 all.gene_end.data(), all.flags.data(), all.code.data(), all.level.data(), h_.out()),
              "abn_windows_create");
    fetch();
  }
  abn_windows* get() const { return h_.get(); }
  size_t n_samples() const { return n_; }
  size_t n_windows() const { return W_; }
  std::vector<int64_t> count, kept;  // [n_samples x W]
  std::vector<double> level_sum, level_sum_kept;
  std::vector<int32_t> ragged;  // [W]

 private:
  void fetch() {  // what the handle reports, to the vectors above
    int32_t W = 0;
    abn_windows_info(get(), &W, nullptr, nullptr);
    W_ = (size_t)W;
    count.resize(n_ * W_);
    kept.resize(n_ * W_);
    level_sum.resize(n_ * W_);
    level_sum_kept.resize(n_ * W_);
    ragged.resize(W_);
    abn_windows_stats(get(), count.data(), level_sum.data(), level_sum_kept.data(), kept.data());
    abn_windows_layout(get(), nullptr, nullptr, ragged.data());
  }
  Owned<abn_windows, abn_windows_destroy> h_;
  size_t n_ = 0, W_ = 0;
};

}  // namespace windows

namespace detail {
inline std::vector<Site> parse_sites_device_reduced(const std::string& text) {
  std::vector<Site> out;
  for (const auto& s : windows::parse_sites_device(default_device(), text, /*skip_lines=*/0))
    out.push_back(Site{s.posteriormax, s.status_numeric, s.meth_lvl});
  return out;
}
}  // namespace detail
}  // namespace alphabeta

#include "resident.hpp"
