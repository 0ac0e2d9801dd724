// Tiny C shim over the C++ host layer so that the Python tests can call Pedigree::build / from_file /
// to_file and the number formatter without a GPU.  Not part of the product ABI (include/abneutral.h).
#include <chrono>
#include <cstring>
#include <memory>

#include "../csrc/abn_genes.hpp"
#include "../csrc/abn_parse.hpp"
#include "../csrc/abn_route.hpp"
#include "../csrc/abn_codes.hpp"
#include "../csrc/abn_pairwise_transitions.hpp"
#include "../csrc/abn_sites_merge.hpp"
#include "../csrc/abn_sites_split.hpp"
#include "../csrc/abn_sites_sort.hpp"
#include "../csrc/abn_sites_dedup.hpp"
// hipcc compiles this file as HIP, device pass included: abn_philox.h (through abn_sim.hpp) names a device function of the
// runtime header there.  (A plain C++ compiler builds this file too, without HIP's include path: tests/test_host_sanitizers.py)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "../csrc/abn_packed_census.hpp"
#include "../csrc/abn_regions.hpp"
#include "../csrc/abn_sim.hpp"
#include "../csrc/abn_sites_common.hpp"
#include "../csrc/abn_sites_union.hpp"
#include "../csrc/abn_tiles.hpp"
#include "alphabeta.hpp"
#include "tiles.hpp"

namespace {
// What the host layer would print (detail::diag_printf) goes into `text` while this lives; the sink it found is put back.
struct DiagCapture {
  std::string text;
  std::string* const found = alphabeta::detail::diag_sink();
  DiagCapture() { alphabeta::detail::diag_sink() = &text; }
  ~DiagCapture() { alphabeta::detail::diag_sink() = found; }
};
struct Stopwatch {  // wall milliseconds since it was made
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
void put_text(char* out, long long cap, const std::string& s) {  // cut to the buffer, always terminated
  if (out && cap > 0) std::strncpy(out, s.c_str(), (size_t)cap - 1), out[cap - 1] = 0;
}
int failed(char* err, int errcap, const std::exception& e) {  // the exception's words for the caller; the shims' -1
  put_text(err, errcap, e.what());
  return -1;
}
}  // namespace

extern "C" {
// returns the number of rows (<0 on error); rows (capacity cap x 4) and *p0uu are filled.  resident: --parse device --sites device
static int pedigree_build(const char* nodelist, const char* edgelist, double posterior_max_filter, bool gpu_pairwise, bool resident,
                          const char* out_path, double* rows, int cap, double* p0uu, char* err, int errcap) {
  try {
    auto [ped, p0] = alphabeta::Pedigree::build(nodelist, edgelist, posterior_max_filter, gpu_pairwise, resident, resident);
    if (out_path) ped.to_file(out_path);
    const int n = (int)ped.nrows();
    if (n > cap) return -2;
    if (n > 0) std::memcpy(rows, ped.data.data(), sizeof(double) * 4 * (size_t)n);  // an empty pedigree has no buffer
    *p0uu = p0;
    return n;
  } catch (const std::exception& e) {
    return failed(err, errcap, e);
  }
}
int abh_pedigree_build(const char* nodelist, const char* edgelist, double posterior_max_filter, double* rows, int cap,
                       double* p0uu, char* err, int errcap) {
  return pedigree_build(nodelist, edgelist, posterior_max_filter, false, false, nullptr, rows, cap, p0uu, err, errcap);
}
// the same with the scan on the GPU, as the `alphabeta` CLI builds its pedigree; out_path (nullable): Pedigree::to_file
int abh_pedigree_build_gpu(const char* nodelist, const char* edgelist, double posterior_max_filter, const char* out_path,
                           double* rows, int cap, double* p0uu, char* err, int errcap) {
  return pedigree_build(nodelist, edgelist, posterior_max_filter, true, false, out_path, rows, cap, p0uu, err, errcap);
}
// scans Pedigree::build has sent through abn_pairwise_divergence_packed since the library was loaded
long long abh_packed_scan_calls() { return alphabeta::detail::packed_scan_calls().load(); }
// ... and calls Pedigree::build_many has sent through abn_pairwise_divergence_windows_packed
long long abh_packed_windows_scan_calls() { return alphabeta::detail::packed_windows_scan_calls().load(); }
// ... and builds whose codes and rc_meth_lvl folds were made on the device from resident sites (--sites device)
long long abh_resident_build_calls() { return alphabeta::detail::resident_build_calls().load(); }
// Pedigree::build as `alphabeta --parse device --sites device` runs it: abh_pedigree_build_gpu's arguments and result
int abh_pedigree_build_resident(const char* nodelist, const char* edgelist, double posterior_max_filter, const char* out_path,
                                double* rows, int cap, double* p0uu, char* err, int errcap) {
  return pedigree_build(nodelist, edgelist, posterior_max_filter, true, true, out_path, rows, cap, p0uu, err, errcap);
}
// The two ways of `alphabeta --parse device` from n methylome texts in host memory (the sampled nodes of the nodelist, in
// its order; the files it names are not opened) to the finished pedigree and p0uu: --sites host (which & 1: the records
// come down, are copied into Site vectors, folded and packed on the host, and the packed matrix goes up) against
// --sites device (which & 2: abn_codes_create_parsed).  which == 3: 1 when rows and p0uu are equal bit for bit, 0 when
// not.  ms2 = the wall time of the two; kernel_ms4 = abn_codes_kernel_ms of the device side.  The texts are kept when
// n > 0: the timed calls pass n = 0.  -1: a call threw (its text in err)
int abh_pedigree_build_ab(const char* nodelist, const char* edgelist, const char* const* texts, const long long* lens, int n,
                          double posterior_max_filter, int which, double* ms2, double* kernel_ms4, char* err, int errcap) {
  try {
    static std::vector<std::string> held;
    if (n > 0) {
      held.clear();
      for (int i = 0; i < n; ++i) held.emplace_back(texts[i], (size_t)lens[i]);
    }
    DiagCapture quiet;  // (both sides print the invalid-status warnings; kept off the console)
    std::pair<alphabeta::Pedigree, double> host, device;
    if (which & 1) {
      const Stopwatch watch;
      host = alphabeta::detail::build_pedigree(nodelist, edgelist, posterior_max_filter, true, true, false, &held);
      ms2[0] = watch.ms();
    }
    if (which & 2) {
      const Stopwatch watch;
      device = alphabeta::detail::build_pedigree(nodelist, edgelist, posterior_max_filter, true, true, true, &held);
      ms2[1] = watch.ms();
      std::memcpy(kernel_ms4, alphabeta::detail::resident_kernel_ms(), 4 * sizeof(double));
    }
    if ((which & 3) != 3) return 1;
    const auto &a = host.first.data, &b = device.first.data;
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), 8 * a.size()) == 0) &&
                   std::memcmp(&host.second, &device.second, 8) == 0
               ? 1
               : 0;
  } catch (const std::exception& e) {
    return failed(err, errcap, e);
  }
}
// The layout of Pedigree::build_many's scan calls without a device: the n entries are read, those that the scan takes
// (samples of equal length, at least two) and that have the first such entry's sample count are cut into calls of at
// most cap_bytes of packed codes (PackedBatch) and every call is laid out (layout_packed_call).  Per entry: call_of (-1:
// not in the scan), n_samples, n_sites, begin / end (sites, in its call's rows), codes_off (where its write_codes bytes
// [samples x sites] start in codes_out).  Per call: stride, packed_off (where its matrix [samples x stride] starts in
// packed_out).  An entry that cannot be read: n_samples -1.
// Returns the number of calls; -1: the call itself threw; -2: a buffer is too small.
int abh_build_many_layout(const char* const* nodelists, const char* const* edgelists, int n, double posterior_max_filter,
                          long long cap_bytes, int* call_of, int* n_samples, long long* n_sites, long long* begin,
                          long long* end, long long* codes_off, unsigned char* codes_out, long long codes_cap,
                          long long* stride, long long* packed_off, unsigned char* packed_out, long long packed_cap) {
  using namespace alphabeta::detail;
  try {
    std::vector<Inputs> in((size_t)n);
    std::vector<PackedBatch> calls;
    size_t nn = 0, codes_used = 0;
    for (int i = 0; i < n; ++i) {
      call_of[i] = -1;
      n_samples[i] = -1;
      n_sites[i] = begin[i] = end[i] = codes_off[i] = 0;
      try {
        in[(size_t)i] = read_inputs(nodelists[i], edgelists[i], posterior_max_filter);
      } catch (const std::exception&) {
        continue;  // (build_many keeps the text; here the entry is simply not in the scan)
      }
      const Inputs& e = in[(size_t)i];
      n_samples[i] = (int)e.nodes.size();
      n_sites[i] = e.nodes.empty() ? 0 : (long long)e.nodes[0].sites.size();
      if (!e.same_len() || e.nodes.size() < 2 || (nn && e.nodes.size() != nn)) continue;
      nn = e.nodes.size();
      const size_t L = e.nodes[0].sites.size();
      if (calls.empty() || !calls.back().takes(L, (size_t)cap_bytes)) {
        calls.emplace_back();
        calls.back().nn = nn;
      }
      calls.back().add((size_t)i, L);
      call_of[i] = (int)calls.size() - 1;
      codes_off[i] = (long long)codes_used;
      if (codes_used + nn * L > (size_t)codes_cap) return -2;
      write_codes(e, posterior_max_filter, codes_out + codes_used, L);
      codes_used += nn * L;
    }
    size_t packed_used = 0;
    for (size_t k = 0; k < calls.size(); ++k) {
      std::vector<const Inputs*> entries;
      for (size_t w : calls[k].members) entries.push_back(&in[w]);
      const PackedCall c = layout_packed_call(calls[k], entries, posterior_max_filter);
      if (packed_used + c.packed.size() > (size_t)packed_cap) return -2;
      std::memcpy(packed_out + packed_used, c.packed.data(), c.packed.size());
      stride[k] = (long long)c.stride;
      packed_off[k] = (long long)packed_used;
      packed_used += c.packed.size();
      for (size_t m = 0; m < calls[k].members.size(); ++m) {
        begin[calls[k].members[m]] = c.begin[m];
        end[calls[k].members[m]] = c.end[m];
      }
    }
    return (int)calls.size();
  } catch (const std::exception&) {
    return -1;
  }
}
// Pedigree::build_many over n (nodelist, edgelist) pairs: per entry the number of rows (-1: failed, its text in
// errs + i * errcap; -2: more than cap rows), rows (n x cap x 4) and p0uu (n); returns 0, or -1 when the call itself threw
int abh_pedigree_build_many(const char* const* nodelists, const char* const* edgelists, int n, double posterior_max_filter,
                            int gpu_pairwise, double* rows, int cap, double* p0uu, int* nrows, char* errs, int errcap) {
  try {
    std::vector<std::pair<std::string, std::string>> lists;
    for (int i = 0; i < n; ++i) lists.push_back({nodelists[i], edgelists[i]});
    const auto built = alphabeta::Pedigree::build_many(lists, posterior_max_filter, gpu_pairwise != 0);
    for (int i = 0; i < n; ++i) {
      const auto& b = built[(size_t)i];
      char* err = errs + (size_t)i * (size_t)errcap;
      if (errcap > 0) err[0] = 0;
      std::fputs(b.diagnostics.c_str(), stdout);
      if (!b.ok) {
        put_text(err, errcap, b.error);
        nrows[i] = -1;
        continue;
      }
      const int r = (int)b.pedigree.nrows();
      nrows[i] = r > cap ? -2 : r;
      if (r > 0 && r <= cap) std::memcpy(rows + (size_t)i * (size_t)cap * 4, b.pedigree.data.data(), sizeof(double) * 4 * (size_t)r);
      p0uu[i] = b.p0uu;
    }
    return 0;
  } catch (const std::exception&) {
    return -1;
  }
}
// ---- the host half of the window extraction (windows_extract.hpp), for tests/test_windows_host.py
// parse_annotation -> the genes of every list as lines "chromosome list start end strand name\n" (list: s / a / c; strand
// 0 / 1 / 2 = + / - / *), chromosomes ascending (256 = M, 257 = C); out2 = {genes parsed, max gene length}.
// Returns the text's length, or -1 when it does not fit
long long abh_annotation_lists(const char* text, long long len, char* out, long long cap, long long* out2) {
  const auto g = alphabeta::windows::parse_annotation(std::string(text, (size_t)len));
  std::string s;
  for (const auto& kv : g.chromosomes) {
    const std::pair<const char*, const std::vector<alphabeta::windows::Gene>*> lists[3] = {
        {"s", &kv.second.sense}, {"a", &kv.second.antisense}, {"c", &kv.second.combined}};
    for (const auto& l : lists)
      for (const auto& e : *l.second)
        s += std::to_string(kv.first) + " " + l.first + " " + std::to_string(e.start) + " " + std::to_string(e.end) + " " +
             std::to_string((int)e.strand) + " " + e.name + "\n";
  }
  out2[0] = (long long)g.n_genes;
  out2[1] = (long long)g.max_gene_length;
  if ((long long)s.size() + 1 > cap) return -1;
  std::memcpy(out, s.c_str(), s.size() + 1);
  return (long long)s.size();
}
// choose_genes of one methylome text against an annotation text -> the per-site arrays abn_windows_create takes (capacity
// cap sites each).  Returns the number of sites, -1 when they do not fit
long long abh_choose_genes(const char* annotation, long long alen, const char* methylome, long long mlen, unsigned cutoff,
                           int cutoff_gene_length, double posterior_max_filter, long long cap, unsigned* pos,
                           unsigned* gene_start, unsigned* gene_end, unsigned char* flags, unsigned char* code,
                           double* level) {
  namespace w = alphabeta::windows;
  const auto g = w::parse_annotation(std::string(annotation, (size_t)alen));
  const auto s = w::choose_genes(std::string(methylome, (size_t)mlen), g, w::GeneRule{cutoff, cutoff_gene_length != 0},
                                 posterior_max_filter);
  const size_t n = s.size();
  if ((long long)n > cap) return -1;
  if (n == 0) return 0;
  std::memcpy(pos, s.pos.data(), 4 * n);
  std::memcpy(gene_start, s.gene_start.data(), 4 * n);
  std::memcpy(gene_end, s.gene_end.data(), 4 * n);
  std::memcpy(flags, s.flags.data(), n);
  std::memcpy(code, s.code.data(), n);
  std::memcpy(level, s.level.data(), 8 * n);
  return (long long)n;
}
// parsed sites and their lines into the caller's arrays (capacity cap) -> their number, -1 when they do not fit
static long long put_sites(const std::vector<alphabeta::windows::FullSite>& sites, const std::vector<int64_t>& lines,
                           long long cap, long long* line, int* chromosome, unsigned* start, unsigned* end,
                           unsigned char* strand, double* posteriormax, unsigned char* status, double* meth_lvl) {
  if ((long long)sites.size() > cap) return -1;
  for (size_t i = 0; i < sites.size(); ++i) {
    line[i] = lines[i];
    chromosome[i] = sites[i].chromosome;
    start[i] = sites[i].start;
    end[i] = sites[i].end;
    strand[i] = (unsigned char)sites[i].strand;
    posteriormax[i] = sites[i].posteriormax;
    status[i] = (unsigned char)sites[i].status_numeric;
    meth_lvl[i] = sites[i].meth_lvl;
  }
  return (long long)sites.size();
}
// ---- the methylome line parser: the host's (parse_site_full) and the one the device shares (csrc/abn_parse.hpp), for
// tests/test_parse_cpu.py and tests/test_parse_gpu.py
// parse_sites_host of a text from line `skip_lines` on -> per site (capacity cap): line, chromosome, start, end, strand,
// posteriormax, status, meth_lvl; *n_warnings = the invalid-status warnings it would have printed.  Returns the number of
// sites, -1 when they do not fit
long long abh_parse_sites(const char* text, long long len, long long skip_lines, long long cap, long long* line,
                          int* chromosome, unsigned* start, unsigned* end, unsigned char* strand, double* posteriormax,
                          unsigned char* status, double* meth_lvl, long long* n_warnings) {
  DiagCapture warnings;
  std::vector<int64_t> lines;
  const auto sites = alphabeta::windows::parse_sites_host(std::string(text, (size_t)len), (size_t)skip_lines, &lines);
  if (n_warnings) *n_warnings = (long long)std::count(warnings.text.begin(), warnings.text.end(), '\n');
  return put_sites(sites, lines, cap, line, chromosome, start, end, strand, posteriormax, status, meth_lvl);
}
// abn::abn_parse_f64 of one token -> 0 value (in *value), 1 rejected, 2 deferred
int abh_parse_f64_token(const char* token, long long len, double* value) {
  const unsigned char* p = (const unsigned char*)token;
  return abn::abn_parse_f64(p, p + len, *value);
}
// abn::abn_parse_line of every line of a text from line `skip_lines` on, as the device walks it (a line per '\n', a last
// line without one, the '\r' trimmed) -> cls[line - skip_lines] = 0 no site, 1 site, 2 deferred (capacity cap lines), and
// per site in file order: u6 = chromosome, start, end, strand, status, status_flag; d2 = posteriormax, meth_lvl; its line
// in site_line.  Returns the number of lines classified, -1 when they do not fit
long long abh_classify_text(const char* text, long long len, long long skip_lines, long long cap, unsigned char* cls,
                            long long* site_line, unsigned* u6, double* d2, long long* n_sites) {
  const unsigned char* t = (const unsigned char*)text;
  long long li = 0, out = 0, ns = 0;
  for (long long b = 0; b < len; ++li) {
    long long e = b;
    while (e < len && t[e] != '\n') ++e;
    if (li >= skip_lines) {
      if (out >= cap) return -1;
      abn::ParsedSite s{};
      const int c = abn::abn_parse_line(t + b, abn::abn_line_trim(t + b, t + e), s);
      cls[out++] = (unsigned char)c;
      if (c == abn::kLineSite) {
        site_line[ns] = li;
        const unsigned u[6] = {(unsigned)s.chromosome, s.start, s.end, s.strand, s.status, s.status_flag};
        std::memcpy(u6 + 6 * ns, u, sizeof u);
        d2[2 * ns] = s.posteriormax;
        d2[2 * ns + 1] = s.meth_lvl;
        ++ns;
      }
    }
    b = e + 1;
  }
  *n_sites = ns;
  return out;
}
// ---- the same two parsers under a context mask (1 CG, 2 CHG, 4 CHH), and the serial form of the partition by context
// (csrc/abn_sites_split.hpp), for tests/test_sites_split_cpu.py and tests/test_sites_split_gpu.py
// abh_parse_sites with parse_sites_host's mask; context (capacity cap) = every site's code
long long abh_parse_sites_ctx(const char* text, long long len, long long skip_lines, unsigned contexts, long long cap,
                              long long* line, int* chromosome, unsigned* start, unsigned* end, unsigned char* strand,
                              double* posteriormax, unsigned char* status, double* meth_lvl, unsigned char* context,
                              long long* n_warnings) {
  DiagCapture warnings;
  std::vector<int64_t> lines;
  const auto sites =
      alphabeta::windows::parse_sites_host(std::string(text, (size_t)len), (size_t)skip_lines, &lines, contexts);
  if (n_warnings) *n_warnings = (long long)std::count(warnings.text.begin(), warnings.text.end(), '\n');
  const long long n = put_sites(sites, lines, cap, line, chromosome, start, end, strand, posteriormax, status, meth_lvl);
  for (long long i = 0; i < n; ++i) context[i] = sites[(size_t)i].context;
  return n;
}
// abh_classify_text with abn_parse_line's mask; site_context = every site's code
long long abh_classify_text_ctx(const char* text, long long len, long long skip_lines, unsigned contexts, long long cap,
                                unsigned char* cls, long long* site_line, unsigned* u6, double* d2,
                                unsigned char* site_context, long long* n_sites) {
  const unsigned char* t = (const unsigned char*)text;
  long long li = 0, out = 0, ns = 0;
  for (long long b = 0; b < len; ++li) {
    long long e = b;
    while (e < len && t[e] != '\n') ++e;
    if (li >= skip_lines) {
      if (out >= cap) return -1;
      abn::ParsedSite s{};
      const int c = abn::abn_parse_line(t + b, abn::abn_line_trim(t + b, t + e), s, contexts);
      cls[out++] = (unsigned char)c;
      if (c == abn::kLineSite) {
        site_line[ns] = li;
        const unsigned u[6] = {(unsigned)s.chromosome, s.start, s.end, s.strand, s.status, s.status_flag};
        std::memcpy(u6 + 6 * ns, u, sizeof u);
        d2[2 * ns] = s.posteriormax;
        d2[2 * ns + 1] = s.meth_lvl;
        site_context[ns] = (unsigned char)s.context;
        ++ns;
      }
    }
    b = e + 1;
  }
  *n_sites = ns;
  return out;
}
// The partition of one sample's records by context under the parent's mask, serially: n_chunks chunks of chunk_n records, their six record arrays
// concatenated (n records in all) -> size [n_chunks * 3] = the records of chunk c in child k at c * 3 + k, and child k's
// arrays, its chunks concatenated, from k * n on in the six output arrays (capacity 3 * n each).  Returns the workgroups
// walked, -1 when the scanned counts and the sizes disagree
long long abh_sites_split_serial(int n_chunks, unsigned contexts, const long long* chunk_n, const unsigned* line, const unsigned* meta,
                                 const unsigned* start, const unsigned* end, const double* pm, const double* ml,
                                 unsigned* size, unsigned* oline, unsigned* ometa, unsigned* ostart, unsigned* oend,
                                 double* opm, double* oml) {
  std::vector<abn::SplitChunk> chunks((size_t)n_chunks);
  long long n = 0, n_blocks = 0;
  for (int c = 0; c < n_chunks; ++c) {
    chunks[(size_t)c].src = abn::MergeChunk{line + n, meta + n, start + n, end + n, pm + n, ml + n, chunk_n[c], 0, 0, n};
    chunks[(size_t)c].block0 = n_blocks;
    n += chunk_n[c];
    n_blocks += abn::split_blocks(chunk_n[c]);
  }
  const long long stride = n_blocks + 1;
  std::vector<uint32_t> count((size_t)(abn::kSplitChildren * stride), 0u);
  abn::split_count_serial(chunks.data(), n_chunks, contexts, count.data(), stride);
  abn::split_scan_serial(count.data(), n_blocks, stride);
  long long at[abn::kSplitChildren] = {0, 0, 0};
  for (int c = 0; c < n_chunks; ++c)
    for (int k = 0; k < abn::kSplitChildren; ++k) {
      const uint32_t s = abn::split_chunk_size(chunks.data(), n_chunks, c, k, count.data(), stride, n_blocks);
      size[c * abn::kSplitChildren + k] = s;
      const long long o = (long long)k * n + at[k];
      chunks[(size_t)c].out[k] = abn::SplitOut{oline + o, ometa + o, ostart + o, oend + o, opm + o, oml + o};
      at[k] += s;
    }
  for (int k = 0; k < abn::kSplitChildren; ++k)
    if (at[k] != (long long)count[(size_t)(k * stride + n_blocks)]) return -1;
  abn::split_scatter_serial(chunks.data(), n_chunks, contexts, count.data(), stride, n_blocks);
  return n_blocks;
}
// ---- the sort by genomic position (csrc/abn_sites_sort.hpp) in its serial forms, for tests/test_sites_sort_cpu.py,
// tests/test_sites_sort_gpu.py and scripts/sort_ab.py
// abn_sites_sort_keys on the host: order [n] = the stable permutation into canonical order, info4 = {n, descents, equal
// neighbours, the radix passes the device would run}.  1: a chromosome outside 0..257, a strand above 2, n < 0 or >= 2^32
int abn_sites_sort_keys_host(long long n, const int* chromosome, const unsigned* start, const unsigned* end,
                             const unsigned char* strand, long long* order, long long* info4) {
  if (n < 0 || n >= (1ll << 32)) return 1;
  for (long long i = 0; i < n; ++i)
    if (!abn::sort_key_valid(chromosome[i], strand[i])) return 1;
  std::vector<abn::SortPair> pair((size_t)n);
  const abn::SortCheck check = abn::sort_check_serial(n, chromosome, start, end, strand, pair.data());
  abn::sort_pairs_serial(pair.data(), n);
  for (long long k = 0; k < n; ++k) order[k] = pair[(size_t)k].index;
  info4[0] = n, info4[1] = check.descents, info4[2] = check.equal, info4[3] = abn::sort_passes_needed(check);
  return 0;
}
// ... as the kernels walk it (sort_walk_serial): tile histograms, row scans and the scatter's ranks from per-wavefront
// counts; skip 0 runs every pass of an input with a descent.  info4[3] = the passes run
int abh_sites_sort_walk(long long n, const int* chromosome, const unsigned* start, const unsigned* end,
                        const unsigned char* strand, int skip, long long* order, long long* info4) {
  std::vector<abn::SortPair> a((size_t)n), b((size_t)n);
  const abn::SortCheck check = abn::sort_check_serial(n, chromosome, start, end, strand, a.data());
  int passes = 0;
  const abn::SortPair* r = abn::sort_walk_serial(a.data(), b.data(), n, check, skip != 0, &passes);
  for (long long k = 0; k < n; ++k) order[k] = r[k].index;
  info4[0] = n, info4[1] = check.descents, info4[2] = check.equal, info4[3] = passes;
  return 0;
}
// the digit pass `pass` reads of a key; the scatter kernel's tile; the passes of the whole key
unsigned abh_sites_sort_digit(int chromosome, unsigned start, unsigned end, unsigned strand, int pass) {
  return abn::sort_digit(abn::sort_key((unsigned)chromosome, start, end, strand).w, pass);
}
int abh_sites_sort_tile() { return abn::kSortTile; }
int abh_sites_sort_passes() { return abn::kSortPasses; }
// ---- the collapse of repeated sites (csrc/abn_sites_dedup.hpp) in its serial forms, for tests/test_sites_dedup_cpu.py,
// tests/test_sites_dedup_gpu.py and scripts/dedup_ab.py
// abn_sites_dedup_keys on the host: order (room for n) = the kept records' indices, info4 = {n, kept, repeated keys,
// disagreeing neighbours}.  1: a policy outside 0..3, n < 0 or >= 2^32, a null array with n > 0, a chromosome outside
// 0..257, a strand above 2, or a descent — *first_descent (may be null) = the first descending site then, else -1
int abn_sites_dedup_keys_host(long long n, const int* chromosome, const unsigned* start, const unsigned* end,
                              const unsigned char* strand, const double* posteriormax, const unsigned char* status, int policy,
                              long long* order, long long* info4, long long* first_descent) {
  long long descent = -1;
  if (first_descent) *first_descent = -1;
  if (n < 0 || n >= (1ll << 32) || !abn::dedup_policy_valid(policy) || !info4) return 1;
  if (n > 0 && (!chromosome || !start || !end || !strand || !posteriormax || !status || !order)) return 1;
  const int rc = abn::dedup_serial(abn::DedupArrays{chromosome, start, end, strand, posteriormax, status}, n, policy, order, info4,
                                   &descent);
  if (first_descent) *first_descent = descent;
  return rc;
}
// ... as the kernels walk it: the flags lane by lane with the striding of `blocks` workgroups, BEST's walk from the head's
// lane, the tile counts, their scan and the scatter's ranks.  info4 as above; check4 = the flags' partial records added up:
// first descent (-1: none), bad keys, repeated keys, disagreeing neighbours.  Nothing is refused: order is what the
// kernels would write
int abh_sites_dedup_walk(long long n, const int* chromosome, const unsigned* start, const unsigned* end,
                         const unsigned char* strand, const double* posteriormax, const unsigned char* status, int policy,
                         long long blocks, long long* order, long long* info4, long long* check4) {
  const abn::DedupArrays keys{chromosome, start, end, strand, posteriormax, status};
  std::vector<uint8_t> keep((size_t)n);
  std::vector<uint32_t> count((size_t)abn::sort_tiles(n) + 1);
  const abn::DedupCheck check = abn::dedup_flags_walk(keys, n, policy, blocks, keep.data());
  const long long kept = abn::dedup_compact_walk(keep.data(), n, count.data(), order);
  info4[0] = n, info4[1] = kept, info4[2] = check.repeated, info4[3] = check.disagreeing;
  check4[0] = check.descent == abn::kDedupNoDescent ? -1 : (long long)check.descent;
  check4[1] = check.bad, check4[2] = check.repeated, check4[3] = check.disagreeing;
  return 0;
}
// parse_sites_device of a text on the default device (slab_bytes as abn_sites_params) -> the arrays of abh_parse_sites;
// warnings (capacity wcap) = what it printed.  Returns the number of sites, -1: they do not fit, -2: the call threw
long long abh_parse_sites_device(const char* text, long long len, long long skip_lines, long long slab_bytes,
                                 long long cap, long long* line, int* chromosome, unsigned* start, unsigned* end,
                                 unsigned char* strand, double* posteriormax, unsigned char* status, double* meth_lvl,
                                 char* warnings_out, long long wcap) {
  try {
    DiagCapture warnings;
    std::vector<int64_t> lines;
    const auto sites = alphabeta::windows::parse_sites_device(alphabeta::default_device(), std::string(text, (size_t)len),
                                                              (size_t)skip_lines, slab_bytes, &lines);
    put_text(warnings_out, wcap, warnings.text);
    return put_sites(sites, lines, cap, line, chromosome, start, end, strand, posteriormax, status, meth_lvl);
  } catch (const std::exception&) {
    return -2;
  }
}
// choose_genes_many against choose_genes_many_device on n methylome texts: 1 when every array of every sample is equal,
// 0 when not, -1 when a call threw.  ms2 = the wall time of the two (host on `threads` threads; device with upload,
// kernels, download, deferred merge and gene choice), for scripts/parse_ab.py
int abh_choose_genes_many_ab(const char* annotation, long long alen, const char* const* texts, const long long* lens,
                             int n, unsigned cutoff, double posterior_max_filter, int threads, int which,
                             double* ms2) {
  namespace w = alphabeta::windows;
  try {
    static std::vector<std::string> held;  // the texts of the last call, kept: the timed calls pass n = 0
    static w::Genome genome;
    if (n > 0) {
      held.clear();
      for (int i = 0; i < n; ++i) held.emplace_back(texts[i], (size_t)lens[i]);
      genome = w::parse_annotation(std::string(annotation, (size_t)alen));
    }
    const w::GeneRule rule{cutoff, false};
    std::vector<w::SampleSites> host, dev;
    if (which & 1) {
      const Stopwatch watch;
      host = w::choose_genes_many(held, genome, rule, posterior_max_filter, (size_t)threads);
      ms2[0] = watch.ms();
    }
    if (which & 2) {
      const Stopwatch watch;
      dev = w::choose_genes_many_device(alphabeta::default_device(), held, genome, rule, posterior_max_filter);
      ms2[1] = watch.ms();
    }
    if (which != 3) return 1;
    for (size_t s = 0; s < held.size(); ++s) {
      const auto &a = host[s], &b = dev[s];
      if (a.pos != b.pos || a.gene_start != b.gene_start || a.gene_end != b.gene_end || a.flags != b.flags ||
          a.code != b.code || a.level.size() != b.level.size() ||
          (!a.level.empty() && std::memcmp(a.level.data(), b.level.data(), 8 * a.level.size()) != 0))
        return 0;
    }
    return 1;
  } catch (const std::exception&) {
    return -1;
  }
}
// ---- the gene choice in blocks (csrc/abn_genes.hpp), for tests/test_genes_cpu.py and scripts/genes_ab.py
// The three phases the device runs, in their serial form on the host, with blocks of block_sites sites: n methylome texts
// (the header row skipped) against an annotation text -> gene_start, gene_end, flags over all samples' sites (capacity cap)
// and site_offset [n + 1].  Returns the number of sites, -1 when they do not fit, -2 for a block length outside 1..65534
long long abh_choose_genes_blocked(const char* annotation, long long alen, const char* const* texts, const long long* lens,
                                   int n, unsigned cutoff, int cutoff_gene_length, int block_sites, long long cap,
                                   long long* site_offset, unsigned* gene_start, unsigned* gene_end, unsigned char* flags) {
  namespace w = alphabeta::windows;
  if (block_sites < 1 || block_sites > 65534) return -2;
  const w::GeneLists l = w::flatten_genome(w::parse_annotation(std::string(annotation, (size_t)alen)));
  std::vector<std::vector<w::FullSite>> samples;
  for (int i = 0; i < n; ++i) samples.push_back(w::parse_sites_host(std::string(texts[i], (size_t)lens[i])));
  const w::SiteArrays a = w::site_arrays(samples, 0.0);
  const size_t S = a.start.size(), cells = (size_t)abn::kGeneChromosomes * abn::kGeneKinds;
  for (int i = 0; i <= n; ++i) site_offset[i] = a.offset[(size_t)i];
  if ((long long)S > cap) return -1;
  std::vector<uint32_t> off(cells, 0), cnt(cells, 0);
  std::vector<uint16_t> chrom(l.start.size());
  for (size_t k = 0; k < l.list_kind.size(); ++k) {
    const size_t cell = (size_t)l.list_chromosome[k] * abn::kGeneKinds + (size_t)l.list_kind[k];
    off[cell] = (uint32_t)l.list_offset[k];
    cnt[cell] = (uint32_t)(l.list_offset[k + 1] - l.list_offset[k]);
    for (int64_t g = l.list_offset[k]; g < l.list_offset[k + 1]; ++g) chrom[(size_t)g] = (uint16_t)l.list_chromosome[k];
  }
  const abn::GeneTable T{off.data(), cnt.data(), chrom.data(), l.start.data(), l.end.data(), l.strand.data()};
  const abn::GeneSites sites{a.chromosome.data(), a.start.data(), a.end.data(), a.strand.data()};
  std::vector<uint32_t> F(S);
  std::vector<uint16_t> next(S), last(S);
  abn::genes_choose_blocked(sites, a.offset.data(), n, T, abn::GeneRule{cutoff, cutoff_gene_length}, block_sites, F.data(),
                            next.data(), last.data(), gene_start, gene_end, flags);
  return (long long)S;
}
// 1 when all that two windows::Handle report and their packed matrices are equal (doubles bit for bit), 0 when not
static int same_handles(alphabeta::Device& dev, const alphabeta::windows::Handle& a, const alphabeta::windows::Handle& b) {
  auto same_bits = [](const std::vector<double>& x, const std::vector<double>& y) {
    return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), 8 * x.size()) == 0);
  };
  if (a.count != b.count || a.kept != b.kept || a.ragged != b.ragged || !same_bits(a.level_sum, b.level_sum) ||
      !same_bits(a.level_sum_kept, b.level_sum_kept))
    return 0;
  int64_t stride[2] = {0, 0};
  abn_windows_info(a.get(), nullptr, &stride[0], nullptr);
  abn_windows_info(b.get(), nullptr, &stride[1], nullptr);
  if (stride[0] != stride[1]) return 0;
  std::vector<uint8_t> pa(a.n_samples() * (size_t)stride[0]), pb(pa.size());
  dev.check(abn_windows_packed(a.get(), pa.data()), "abn_windows_packed");
  dev.check(abn_windows_packed(b.get(), pb.data()), "abn_windows_packed");
  std::vector<int64_t> ba(a.n_windows()), ea(ba.size()), bb(ba.size()), eb(ba.size());
  abn_windows_layout(a.get(), ba.data(), ea.data(), nullptr);
  abn_windows_layout(b.get(), bb.data(), eb.data(), nullptr);
  return pa == pb && ba == bb && ea == eb ? 1 : 0;
}
// The two ways to a windows::Handle from parsed sites, on n methylome texts: choose_genes on `threads` threads and the
// Handle of its arrays (which & 1), against the Handle that chooses on the device (which & 2).  which == 3: 1 when all
// that the two handles report and their packed matrices are equal, 0 when not.  ms2 = the wall time of the two from the
// FullSite vectors to the finished Handle; which & 4: kernel_ms3 = the three kernels' times of abn_genes_choose on the
// same sites.  The texts are parsed (on the host) when n > 0 and kept: the timed calls pass n = 0.  -1: a call threw
int abh_windows_handles_ab(const char* annotation, long long alen, const char* const* texts, const long long* lens, int n,
                           unsigned cutoff, int cutoff_gene_length, double posterior_max_filter, unsigned step,
                           unsigned size, int absolute, int threads, int which, double* ms2, double* kernel_ms3) {
  namespace w = alphabeta::windows;
  try {
    static std::vector<std::vector<w::FullSite>> sites;
    static w::Genome genome;
    if (n > 0) {
      std::vector<std::string> held;
      for (int i = 0; i < n; ++i) held.emplace_back(texts[i], (size_t)lens[i]);
      sites = w::parse_sites_many(held, nullptr, (size_t)threads);
      genome = w::parse_annotation(std::string(annotation, (size_t)alen));
    }
    const w::GeneRule rule{cutoff, cutoff_gene_length != 0};
    const abn_windows_params p =
        w::window_params(cutoff, step, size, absolute != 0, absolute ? genome.max_gene_length : 100u);
    alphabeta::Device& dev = alphabeta::default_device();
    std::unique_ptr<w::Handle> host, device;
    if (which & 1) {
      const Stopwatch watch;
      host = std::make_unique<w::Handle>(dev, p, w::choose_genes_many(sites, genome, rule, posterior_max_filter, (size_t)threads));
      ms2[0] = watch.ms();
    }
    if (which & 2) {
      const Stopwatch watch;
      device = std::make_unique<w::Handle>(dev, p, genome, rule, posterior_max_filter, sites);
      ms2[1] = watch.ms();
    }
    if (which & 4) {
      const w::GenesHandle genes(dev, genome);
      const w::SiteArrays a = w::site_arrays(sites, posterior_max_filter);
      std::vector<uint32_t> gs(a.start.size()), ge(a.start.size());
      std::vector<uint8_t> fl(a.start.size());
      const abn_gene_rule r{cutoff, cutoff_gene_length};
      dev.check(abn_genes_choose(genes.get(), &r, (int32_t)sites.size(), a.offset.data(), a.chromosome.data(),
                                 a.start.data(), a.end.data(), a.strand.data(), gs.data(), ge.data(), fl.data(), kernel_ms3),
                "abn_genes_choose");
    }
    if ((which & 3) != 3) return 1;
    return same_handles(dev, *host, *device);
  } catch (const std::exception&) {
    return -1;
  }
}
// ---- the merge of the parser's records with the host-decided lines (csrc/abn_sites_merge.hpp), for
// tests/test_sites_merge_cpu.py and scripts/resident_ab.py
// sites_merge_serial of one sample: n_chunks chunks of chunk_n records and chunk_lines lines each, their record arrays
// concatenated (line: slab-relative; line0 of a chunk = the lines of the chunks in front plus first_line0), and n_ins
// inserted records (file lines, ascending) -> the six arrays over the merged sequence and the places of the records
// (dest_record) and of the inserted records (dest_inserted).  Returns 0; -1: an inserted line lies in no chunk's slab or
// the lines do not ascend
int abh_sites_merge_serial(int n_chunks, const long long* chunk_n, const long long* chunk_lines, long long first_line0,
                           const unsigned* line, const unsigned* meta, const unsigned* start, const unsigned* end,
                           const double* pm, const double* ml, long long n_ins, const long long* iline, const int* ichrom,
                           const unsigned* istart, const unsigned* iend, const unsigned char* istrand,
                           const unsigned char* istatus, const double* ipm, const double* iml, double filter,
                           int* chromosome, unsigned* out_start, unsigned* out_end, unsigned char* strand,
                           unsigned char* code, double* level, long long* dest_record, long long* dest_inserted) {
  std::vector<abn::MergeChunk> chunks;
  long long before = 0, line0 = first_line0;
  for (int c = 0; c < n_chunks; ++c) {
    chunks.push_back(abn::MergeChunk{line + before, meta + before, start + before, end + before, pm + before, ml + before,
                                     chunk_n[c], line0, chunk_lines[c], before});
    before += chunk_n[c];
    line0 += chunk_lines[c];
  }
  std::vector<int32_t> pick((size_t)n_ins);
  if (!abn::merge_pick_chunks(chunks.data(), n_chunks, iline, n_ins, pick.data())) return -1;
  const abn::MergeInserted ins{iline, pick.data(), ichrom, istart, iend, istrand, istatus, ipm, iml, n_ins};
  abn::sites_merge_serial(chunks.data(), n_chunks, ins, filter,
                          abn::MergeOut{chromosome, out_start, out_end, strand, code, level}, dest_record, dest_inserted);
  return 0;
}
// ---- the pedigree build from resident sites (csrc/abn_codes.hpp), for tests/test_codes_cpu.py
// codes_build_serial of one sample: the chunks and inserted records of abh_sites_merge_serial, reduced to what the build
// reads -> the merged bytes and levels over the merged sequence, the sample's packed row [row_stride_bytes], and the fold
// (sum, kept).  Returns 0; -1: an inserted line lies in no chunk's slab or the lines do not ascend; -2: a row stride that
// is no multiple of 4 or holds fewer fields than sites
int abh_codes_build_serial(int n_chunks, const long long* chunk_n, const long long* chunk_lines, long long first_line0,
                           const unsigned* line, const unsigned* meta, const double* pm, const double* ml, long long n_ins,
                           const long long* iline, const unsigned char* istatus, const double* ipm, const double* iml,
                           double filter, long long row_stride_bytes, unsigned char* code, double* level,
                           unsigned char* row, double* sum, long long* kept) {
  std::vector<abn::MergeChunk> chunks;
  long long before = 0, line0 = first_line0;
  for (int c = 0; c < n_chunks; ++c) {
    chunks.push_back(abn::MergeChunk{line + before, meta + before, nullptr, nullptr, pm + before, ml + before, chunk_n[c],
                                     line0, chunk_lines[c], before});
    before += chunk_n[c];
    line0 += chunk_lines[c];
  }
  if (row_stride_bytes < 0 || row_stride_bytes % 4 != 0 || 4 * row_stride_bytes < before + n_ins) return -2;
  std::vector<int32_t> pick((size_t)n_ins);
  if (!abn::merge_pick_chunks(chunks.data(), n_chunks, iline, n_ins, pick.data())) return -1;
  const abn::MergeInserted ins{iline, pick.data(), nullptr, nullptr, nullptr, nullptr, istatus, ipm, iml, n_ins};
  abn::codes_build_serial(chunks.data(), n_chunks, ins, filter, abn::CodesOut{code, level}, row, row_stride_bytes, sum, kept);
  return 0;
}
// ---- the sites every sample shares, by position (csrc/abn_sites_common.hpp), for tests/test_sites_common_cpu.py
// sites_common_serial of n samples (site_off [n + 1]; the key fields concatenated) -> keep [site_off[n]] and the return
// value n_common; or -1 with refusal = {kind (1 split run, 2 not ascending, 3 a key outside its range, 4 not co-ordered),
// sample, the site's index in it} and, when text (capacity cap) is given, the refusal's words.  -2: a null pointer
long long abh_sites_common_serial(int n, const long long* site_off, const int* chromosome, const unsigned* start,
                                  const unsigned* end, const unsigned char* strand, unsigned char* keep,
                                  long long* refusal, char* text, long long cap) {
  if (n <= 0 || !site_off || !refusal || (site_off[n] > 0 && (!chromosome || !start || !end || !strand || !keep))) return -2;
  abn::CommonRefusal r{0, -1, -1};
  const long long n_common = abn::sites_common_serial(abn::CommonSites{chromosome, start, end, strand}, n, site_off, keep, &r);
  refusal[0] = r.kind;
  refusal[1] = r.sample;
  refusal[2] = r.site;
  put_text(text, cap, abn::common_refusal_text(r));
  return n_common;
}
// ---- the union of the samples' sites (csrc/abn_sites_union.hpp), for tests/test_sites_union_cpu.py
// sites_union_serial of n samples (arguments as abh_sites_common_serial) -> dest [site_off[n]] (every site's union rank)
// and the return value n_union; or -1 with refusal = {kind (1 split run, 2 not ascending, 3 a key outside its range, 5 run
// order), sample, the site's index in it} and, when text (capacity cap) is given, the refusal's words.  With gathered != 0
// the gather runs too, into arrays of n x gathered sites (-4 unless gathered = n_union; code_in, level_in [site_off[n]]
// are the sites' codes and levels; any output may be null).  -2: a null pointer; -3: 2^32 sites or more
long long abh_sites_union_serial(int n, const long long* site_off, const int* chromosome, const unsigned* start,
                                 const unsigned* end, const unsigned char* strand, unsigned* dest, long long* refusal,
                                 char* text, long long cap, long long gathered, const unsigned char* code_in,
                                 const double* level_in, int* out_chromosome, unsigned* out_start, unsigned* out_end,
                                 unsigned char* out_strand, unsigned char* out_code, double* out_level) {
  if (n <= 0 || !site_off || !refusal || (site_off[n] > 0 && (!chromosome || !start || !end || !strand || !dest))) return -2;
  if (site_off[n] > 0xffffffffLL) return -3;
  abn::CommonRefusal r{0, -1, -1};
  bool fits = true;
  const long long n_union = abn::sites_union_serial(
      abn::CommonSites{chromosome, start, end, strand}, n, site_off, dest, &r, [&](long long nu) {
        if (gathered == 0) return abn::CommonGather{};
        if (gathered != nu) {
          fits = false;
          return abn::CommonGather{};
        }
        return abn::CommonGather{code_in, level_in, out_chromosome, out_start, out_end, out_strand, out_level, out_code, nu};
      });
  refusal[0] = r.kind;
  refusal[1] = r.sample;
  refusal[2] = r.site;
  put_text(text, cap, abn::union_refusal_text(r));
  return fits ? n_union : -4;
}
// ---- genomic tiles (csrc/abn_tiles.hpp, host/tiles.hpp), for tests/test_tiles_cpu.py
// tiles_runs_serial of the columns' keys -> the run tables run_begin / run_end [258] and the runs in run order (capacity 258
// each); returns n_runs, or -1 with refusal = {kind, sample, site} and the refusal's words in text (capacity cap)
int abh_tiles_runs_serial(long long n_columns, const int* chromosome, const unsigned* start, const unsigned* end,
                          const unsigned char* strand, long long* run_begin, long long* run_end, int* run_chromosome,
                          long long* run_first, long long* run_count, unsigned* run_last_start, long long* refusal,
                          char* text, long long cap) {
  std::vector<abn::TileRun> runs;
  abn::CommonRefusal r{0, -1, -1};
  const bool ok = abn::tiles_runs_serial(abn::CommonSites{chromosome, start, end, strand}, n_columns, run_begin, run_end,
                                         &runs, &r);
  refusal[0] = r.kind, refusal[1] = r.sample, refusal[2] = r.site;
  put_text(text, cap, abn::common_refusal_text(r));
  if (!ok) return -1;
  for (size_t k = 0; k < runs.size(); ++k) {
    run_chromosome[k] = runs[k].chromosome, run_first[k] = runs[k].first, run_count[k] = runs[k].count;
    run_last_start[k] = runs[k].last_start;
  }
  return (int)runs.size();
}
// tiles_fixed_intervals over a run table -> the number of tiles (-1: size <= 0 or step < 0); null outputs: only counted
long long abh_tiles_fixed_intervals(int n_runs, const int* run_chromosome, const unsigned* run_last_start, long long size,
                                    long long step, int* chromosome, long long* start, long long* end) {
  std::vector<abn::TileRun> runs;
  for (int k = 0; k < n_runs; ++k) runs.push_back(abn::TileRun{run_chromosome[k], 0, 0, run_last_start[k]});
  return abn::tiles_fixed_intervals(runs.data(), n_runs, size, step, chromosome, start, end);
}
// 1 when (chromosome, start, end) is a tile abn_tiles_set_intervals takes
int abh_tiles_interval_valid(int chromosome, long long start, long long end) {
  return abn::tiles_interval_valid(chromosome, start, end) ? 1 : 0;
}
void abh_tiles_search_serial(const unsigned* start, const long long* run_begin, const long long* run_end, long long T,
                             const int* chromosome, const long long* pos, const long long* pos_end, long long* begin,
                             long long* end) {
  abn::tiles_search_serial(start, run_begin, run_end, T, chromosome, pos, pos_end, begin, end);
}
void abh_tiles_fold_serial(const unsigned char* code, long long code_stride, const double* level, long long n_columns, int n,
                           long long T, const long long* begin, const long long* end, double* sum, long long* kept) {
  abn::tiles_fold_serial(code, code_stride, level, n_columns, n, T, begin, end, sum, kept);
}
// read_regions of a BED-like text -> the number of tiles (-1: more than cap)
long long abh_tiles_read_regions(const char* text, long long len, long long cap, int* chromosome, long long* start,
                                 long long* end) {
  const alphabeta::metaprofile::TileList l = alphabeta::metaprofile::read_regions(std::string(text, (size_t)len));
  if ((long long)l.size() > cap) return -1;
  for (size_t k = 0; k < l.size(); ++k) chromosome[k] = l.chromosome[k], start[k] = l.start[k], end[k] = l.end[k];
  return (long long)l.size();
}
// <chromosome>:<start>-<end> as results.txt spells a tile
void abh_tiles_region(int chromosome, long long start, long long end, char* text, long long cap) {
  put_text(text, cap, alphabeta::metaprofile::tile_region(chromosome, start, end));
}
// ---- region pools (csrc/abn_tiles.hpp: pools; host/tiles.hpp: region_pools), for tests/test_tile_pools_cpu.py
// tiles_pool_merge over a run table (chromosomes in run order) -> the number of segments (-1: more than cap); the segments'
// pool, chromosome, start, end [cap] and seg_first [n_pools + 1]
long long abh_tiles_pool_merge(int n_runs, const int* run_chromosome, long long n_intervals, const int* chromosome,
                               const long long* start, const long long* end, const int* pool, int n_pools, long long cap,
                               int* seg_pool, int* seg_chromosome, long long* seg_start, long long* seg_end,
                               long long* seg_first) {
  std::vector<abn::TileRun> runs;
  for (int k = 0; k < n_runs; ++k) runs.push_back(abn::TileRun{run_chromosome[k], 0, 0, 0u});
  abn::PoolSegments s;
  abn::tiles_pool_merge(runs.data(), n_runs, n_intervals, chromosome, start, end, pool, n_pools, &s);
  if ((long long)s.size() > cap) return -1;
  for (size_t k = 0; k < s.size(); ++k)
    seg_pool[k] = s.pool[k], seg_chromosome[k] = s.chromosome[k], seg_start[k] = s.start[k], seg_end[k] = s.end[k];
  for (size_t p = 0; p < s.seg_first.size(); ++p) seg_first[p] = s.seg_first[p];
  return (long long)s.size();
}
// seg_off [S + 1] of the segments' columns, the pools' ranges [n_pools] of it, and src [seg_off[S]] when it is given
void abh_tiles_pool_offsets_map(long long S, const long long* col_begin, const long long* col_end, long long* seg_off,
                                long long n_pools, const long long* seg_first, long long* begin, long long* end,
                                long long* src) {
  abn::tiles_pool_offsets_serial(col_begin, col_end, S, seg_off);
  if (seg_first) abn::tiles_pool_ranges_serial(seg_off, seg_first, n_pools, begin, end);
  if (src) abn::tiles_pool_map_serial(seg_off, S, col_begin, src);
}
void abh_tiles_pool_gather_serial(const unsigned char* code, long long code_stride, const double* level, long long n_columns,
                                  int n, const long long* src, long long pooled, unsigned char* pcode, long long pcode_stride,
                                  double* plevel) {
  abn::tiles_pool_gather_serial(code, code_stride, level, n_columns, n, src, pooled, pcode, pcode_stride, plevel);
}
// 1 when a matrix of n rows of `columns` sites is within a handle's limits (its stride: abn_packed_row_stride, at least 64)
int abh_tiles_matrix_fits(int n, long long columns) {
  return abn::tiles_matrix_fits(n, columns, std::max<long long>(abn_packed_row_stride(columns), 64)) ? 1 : 0;
}
// read_regions + region_pools of a BED-like text -> the named rows (-1: more than cap, -2: refused, the words in text): their
// chromosome, start, end, pool [cap]; counts = {pools, skipped rows}; names: the pools' names, '\n' between them
long long abh_tiles_region_pools(const char* bed, long long len, long long cap, int* chromosome, long long* start,
                                 long long* end, int* pool, long long* counts, char* text, long long textcap) {
  const auto p = alphabeta::metaprofile::region_pools(alphabeta::metaprofile::read_regions(std::string(bed, (size_t)len)));
  if (!p.refused.empty()) return put_text(text, textcap, p.refused), -2;
  if ((long long)p.rows.size() > cap) return -1;
  for (size_t k = 0; k < p.rows.size(); ++k)
    chromosome[k] = p.rows.chromosome[k], start[k] = p.rows.start[k], end[k] = p.rows.end[k], pool[k] = p.pool[k];
  counts[0] = (long long)p.names.size(), counts[1] = (long long)p.skipped;
  std::string names;
  for (size_t k = 0; k < p.names.size(); ++k) names += p.names[k] + ":" + std::to_string(p.intervals[k]) + "\n";
  put_text(text, textcap, names);
  return (long long)p.rows.size();
}
// detail::convert(graph, dm) -> rows_a, and detail::rows_from(detail::convert_times(graph), dm) -> rows_b (capacity cap x 4
// each; dm [nn x nn] as DMatrix::from fills it); *nn_out = the sampled nodes.  Returns the rows of convert, -1: a call
// threw, and when both forms ran, both threw the same words (in err), -2: they do not fit, -3: the two differ in their
// number of rows, -4: one form threw and the other did not, or in other words
int abh_tiles_convert_both(const char* nodelist, const char* edgelist, const double* dm, int* nn_out, double* rows_a,
                           double* rows_b, int cap, char* err, int errcap) {
  try {
    const alphabeta::detail::Inputs graph = alphabeta::detail::read_graph(nodelist, edgelist);
    const size_t nn = graph.nodes.size();
    if (nn_out) *nn_out = (int)nn;
    if (!dm) return 0;
    const std::vector<double> d(dm, dm + nn * nn);
    alphabeta::Pedigree a, b;
    std::string threw[2];
    try {
      a = alphabeta::detail::convert(graph, d);
    } catch (const alphabeta::Error& e) {
      threw[0] = e.what();
    }
    try {
      b = alphabeta::detail::rows_from(alphabeta::detail::convert_times(graph), d, nn);
    } catch (const alphabeta::Error& e) {
      threw[1] = e.what();
    }
    if (threw[0] != threw[1]) return -4;
    if (!threw[0].empty()) return put_text(err, errcap, threw[0]), -1;
    if (a.nrows() != b.nrows()) return -3;
    if ((int)a.nrows() > cap) return -2;
    if (a.nrows() > 0) {
      std::memcpy(rows_a, a.data.data(), sizeof(double) * 4 * a.nrows());
      std::memcpy(rows_b, b.data.data(), sizeof(double) * 4 * b.nrows());
    }
    return (int)a.nrows();
  } catch (const std::exception& e) {
    return failed(err, errcap, e);
  }
}
// the comparator the searches share: 1 when key a = (start, end, strand) is below key b, and 1 in *equal when they are the same
int abh_sites_common_key_less(unsigned a_start, unsigned a_end, unsigned a_strand, unsigned b_start, unsigned b_end,
                              unsigned b_strand, int* equal) {
  const abn::CommonKey a{a_start, a_end, a_strand}, b{b_start, b_end, b_strand};
  if (equal) *equal = abn::common_key_equal(a, b) ? 1 : 0;
  return abn::common_key_less(a, b) ? 1 : 0;
}
// parse_sites_resident of a text on the default device -> what abn_sites_fetch gives for its handle, in the arrays of
// abh_parse_sites; warnings (capacity wcap) = what it printed.  Returns the number of sites, -1: they do not fit, -2: the
// call threw
long long abh_parse_sites_resident(const char* text, long long len, long long skip_lines, long long slab_bytes,
                                   long long cap, long long* line, int* chromosome, unsigned* start, unsigned* end,
                                   unsigned char* strand, double* posteriormax, unsigned char* status, double* meth_lvl,
                                   char* warnings_out, long long wcap) {
  try {
    DiagCapture warnings;
    const alphabeta::windows::ResidentSites sites = alphabeta::windows::parse_sites_resident(
        alphabeta::default_device(), std::string(text, (size_t)len), (size_t)skip_lines, slab_bytes);
    put_text(warnings_out, wcap, warnings.text);
    if ((long long)sites.size() > cap) return -1;
    static_assert(sizeof(long long) == sizeof(int64_t), "line numbers");
    alphabeta::default_device().check(
        abn_sites_fetch(sites.get(), (int64_t*)line, chromosome, start, end, strand, posteriormax, status, nullptr, meth_lvl),
        "abn_sites_fetch");
    return (long long)sites.size();
  } catch (const std::exception&) {
    return -2;
  }
}
// The two ways from n methylome texts in host memory to a finished windows::Handle with the genes chosen on the device:
// parse_sites_many on the device and the Handle of its FullSite vectors (which & 1: the records come down, are merged and
// copied twice on the host and go up again), against parse_sites_resident and the Handle of its ResidentSites (which & 2:
// the records stay).  which == 3: 1 when all that the two handles report and their packed matrices are equal, 0 when
// not.  ms2 = the wall time of the two; kernel_ms2 = the HIP-event times of the resident side's two merge kernels.  The
// texts are kept when n > 0: the timed calls pass n = 0.  -1: a call threw
int abh_windows_resident_ab(const char* annotation, long long alen, const char* const* texts, const long long* lens, int n,
                            unsigned cutoff, int cutoff_gene_length, double posterior_max_filter, unsigned step,
                            unsigned size, int absolute, int which, double* ms2, double* kernel_ms2) {
  namespace w = alphabeta::windows;
  try {
    static std::vector<std::string> held;
    static w::Genome genome;
    if (n > 0) {
      held.clear();
      for (int i = 0; i < n; ++i) held.emplace_back(texts[i], (size_t)lens[i]);
      genome = w::parse_annotation(std::string(annotation, (size_t)alen));
    }
    const w::GeneRule rule{cutoff, cutoff_gene_length != 0};
    const abn_windows_params p =
        w::window_params(cutoff, step, size, absolute != 0, absolute ? genome.max_gene_length : 100u);
    alphabeta::Device& dev = alphabeta::default_device();
    DiagCapture quiet;  // (both sides print the invalid-status warnings; kept off the console)
    std::unique_ptr<w::Handle> host, device;
    if (which & 1) {
      const Stopwatch watch;
      host = std::make_unique<w::Handle>(dev, p, genome, rule, posterior_max_filter, w::parse_sites_many(held, &dev));
      ms2[0] = watch.ms();
    }
    if (which & 2) {
      const Stopwatch watch;
      std::vector<w::ResidentSites> sites;
      for (const std::string& text : held) sites.push_back(w::parse_sites_resident(dev, text));
      device = std::make_unique<w::Handle>(dev, p, genome, rule, posterior_max_filter, sites);
      ms2[1] = watch.ms();
      abn_windows_merge_ms(device->get(), kernel_ms2);
    }
    if ((which & 3) != 3) return 1;
    return same_handles(dev, *host, *device);
  } catch (const std::exception&) {
    return -1;
  }
}
// window_params -> out3 = the window counts of upstream, gene, downstream (Windows::new)
void abh_window_counts(unsigned cutoff, unsigned step, unsigned size, int absolute, unsigned max_gene_length, int* out3) {
  const abn_windows_params p = alphabeta::windows::window_params(cutoff, step, size, absolute != 0, max_gene_length);
  out3[0] = p.n_upstream;
  out3[1] = p.n_gene;
  out3[2] = p.n_downstream;
}
int abh_pedigree_roundtrip(const char* in_path, const char* out_path) {
  try {
    auto ped = alphabeta::Pedigree::from_file(in_path);
    ped.to_file(out_path);
    return (int)ped.nrows();
  } catch (const std::exception&) {
    return -1;
  }
}
int abh_fmt_f64(double v, char* out, int cap) {
  const std::string s = alphabeta::fmt_f64(v);
  if ((int)s.size() + 1 > cap) return -1;
  std::memcpy(out, s.c_str(), s.size() + 1);
  return (int)s.size();
}
// RawAnalysis::analyze -> 0 and the mean of alpha, or -1 and the error text (a table with non-finite fits)
int abh_analyze(const double* rows, long long n_boot, double* mean_alpha, char* err, int errcap) {
  try {
    alphabeta::RawAnalysis r;
    r.n_boot = (size_t)n_boot;
    r.rows.assign(rows, rows + 7 * n_boot);
    *mean_alpha = r.analyze().alpha;
    return 0;
  } catch (const std::exception& e) {
    return failed(err, errcap, e);
  }
}
int abh_write_npy(const char* path, const double* rows, long long n_boot) {
  alphabeta::RawAnalysis r;
  r.n_boot = (size_t)n_boot;
  r.rows.assign(rows, rows + 7 * n_boot);
  r.write_npy(path);
  return 0;
}

// The launch policy (csrc/abn_route.hpp) as plain integers, for the CPU tier of tests/test_kernel_matrix_census.py.
// pedigree level -> out[8]: lanes, tree, tree as abn_reduction_tree reports it, streams, a wavefront per chain allowed,
// speculative kernel applies, lanes of abn_cost_batch, selection LDS bytes; returns 1 when abn_plan_create refuses
static abn::PedigreeRoute abh_pedigree(int n, int k, int t, int lanes, int strict) {
  return abn::route_pedigree(n, k, t, lanes, strict);
}
int abh_route_pedigree(int n, int k, int t, int lanes, int strict, long long* out) {
  const abn::PedigreeRoute p = abh_pedigree(n, k, t, lanes, strict);
  const long long v[8] = {p.lanes, p.tree, p.reported_tree, p.streams, p.wide_ok, p.spec_ok, p.cost_lanes, (long long)p.select_lds};
  std::memcpy(out, v, sizeof v);
  return p.refusal ? 1 : 0;
}
// phase level (phase 0 = A, 1 = B; plan_chains: windows x starts or bootstraps) -> out[3]: speculative, lanes, two passes
void abh_route_phase(int n, int k, int t, int lanes, int strict, int phase, long long plan_chains, int cus, int dmode,
                     int whole, int two_pass, int* out) {
  const abn::PhaseRoute r = abn::route_phase(abh_pedigree(n, k, t, lanes, strict), phase, plan_chains, cus, dmode, whole != 0, two_pass != 0);
  out[0] = r.spec;
  out[1] = r.lanes;
  out[2] = r.two_pass;
}
// launch level (spec, phase_lanes: the phase level's answer; queue, parking, pass: abn::LaunchOffer) -> out[15]: kind, the key
// (family, G, R, TP, STRICT, RESUME), grid, block, LDS bytes, chain_stride, tree, quantum, tail_cap, RMAX of the tail's
// resume launch (spec<R, tree, resume>; 0: none); returns the status (the text in err)
int abh_route_launch(int n, int k, int t, int lanes, int strict, int spec, int phase_lanes, long long chains, int cus,
                     int queue, int parking, int pass, long long* out, char* err, int errcap) {
  const abn::PedigreeRoute p = abh_pedigree(n, k, t, lanes, strict);
  abn::LaunchOffer o;
  o.queue = queue != 0;
  o.parking = parking != 0;
  o.pass = pass;
  const abn::LaunchRoute r = abn::route_launch(p, abn::PhaseRoute{spec != 0, phase_lanes, false}, chains, cus, o);
  put_text(err, errcap, r.error ? r.error : "");
  const long long v[15] = {r.kind, r.key.family, r.key.G, r.key.R, r.key.tp, r.key.strict, r.key.resume, r.grid, r.block,
                           (long long)r.lds, r.chain_stride, r.tree, r.quantum, r.tail_cap,
                           r.tail_cap > 0 ? abn::route_tail_resume(p, r.tail_cap).key.R : 0};
  std::memcpy(out, v, sizeof v);
  return r.status;
}
// abh_route_launch with abn::LaunchOffer::sweep as one more argument (abn_plan_set_stream_sweep); family 4 is the sweep
// kernel's.  Same out[15].
int abh_route_launch_sweep(int n, int k, int t, int lanes, int strict, int spec, int phase_lanes, long long chains, int cus,
                           int queue, int parking, int pass, int sweep, long long* out, char* err, int errcap) {
  const abn::PedigreeRoute p = abh_pedigree(n, k, t, lanes, strict);
  abn::LaunchOffer o;
  o.queue = queue != 0;
  o.parking = parking != 0;
  o.pass = pass;
  o.sweep = sweep != 0;
  const abn::LaunchRoute r = abn::route_launch(p, abn::PhaseRoute{spec != 0, phase_lanes, false}, chains, cus, o);
  put_text(err, errcap, r.error ? r.error : "");
  const long long v[15] = {r.kind, r.key.family, r.key.G, r.key.R, r.key.tp, r.key.strict, r.key.resume, r.grid, r.block,
                           (long long)r.lds, r.chain_stride, r.tree, r.quantum, r.tail_cap,
                           r.tail_cap > 0 ? abn::route_tail_resume(p, r.tail_cap).key.R : 0};
  std::memcpy(out, v, sizeof v);
  return r.status;
}
// the serial host form of the transitions scan (abn_pairwise_transitions.hpp): table [W][pairs][9] of the windows
// [begin[w], end[w]) of n packed rows of `stride` bytes
void abh_transitions_packed(const unsigned char* packed, int n, long long stride, const long long* begin,
                            const long long* end, int W, unsigned long long* table) {
  const long long pairs = (long long)n * (n - 1) / 2;
  for (int w = 0; w < W; ++w)
    abn::abn_transitions_packed_host(packed, n, stride, begin[w], end[w], (uint64_t*)table + (size_t)w * pairs * 9);
}
// ---- methylomes simulated down a pedigree (csrc/abn_sim.hpp) in their serial forms, for tests/test_sim_cpu.py,
// tests/test_sim_gpu.py and scripts/simulate_ab.py
// abn_sim_codes on the host, site by site: packed [emitted nodes x row_stride].  1 with the refusal's words in `text`
// (text_bytes, may be null): what abn_sim_codes refuses
int abn_sim_codes_host(unsigned long long seed, int n_nodes, const int* parent, const unsigned long long* thr,
                       const unsigned char* emit, long long n_sites, unsigned char* packed, long long row_stride, char* text,
                       int text_bytes) {
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "thresholds");
  const std::string why = abn::sim_refusal(n_nodes, parent, (const uint64_t*)thr, emit, n_sites, packed, row_stride);
  put_text(text, text_bytes, why);
  if (!why.empty()) return 1;
  abn::sim_codes_serial(seed, n_nodes, parent, (const uint64_t*)thr, emit, n_sites, packed, row_stride);
  return 0;
}
// ... as the kernel walks it: `blocks` workgroups of lanes grid-strided over the row's dwords, a lane's trip the nodes in
// index order, unemitted live nodes in scratch rows; lazy = 0: the low words always drawn.  Valid arguments
int abh_sim_codes_walk(unsigned long long seed, int n_nodes, const int* parent, const unsigned long long* thr,
                       const unsigned char* emit, long long n_sites, long long blocks, int lazy, unsigned char* packed,
                       long long row_stride) {
  const abn::SimPlan plan = abn::sim_plan(n_nodes, parent, emit);
  std::vector<uint8_t> scratch((size_t)plan.n_scratch * (size_t)abn::sim_row_bytes(n_sites) + 4);
  if (lazy) abn::sim_codes_walk<true>(seed, n_nodes, plan.nodes.data(), (const uint64_t*)thr, n_sites, blocks, packed, row_stride, scratch.data());
  else abn::sim_codes_walk<false>(seed, n_nodes, plan.nodes.data(), (const uint64_t*)thr, n_sites, blocks, packed, row_stride, scratch.data());
  return 0;
}
long long abh_sim_grid_blocks(long long n_sites, int cus) { return abn::sim_grid_blocks(abn::sim_row_bytes(n_sites) / 4, cus); }
int abh_sim_threads() { return abn::kSimThreads; }
// ---- the observation step and the state census in their host forms, for tests/test_sim_study_cpu.py, test_sim_study_gpu.py
// abn_sim_observe on the host.  walk_blocks = 0: the law site by site; > 0: the kernel's lane function walked over that
// many workgroups' grid stride, lazy = 0 with the low words always drawn.  1 with the refusal's words in `text`
int abn_sim_observe_host(unsigned long long seed, int n_rows, const int* node_of_row, const unsigned long long* othr,
                         long long n_sites, const unsigned char* packed_in, long long in_stride, unsigned char* packed_out,
                         long long out_stride, long long walk_blocks, int lazy, char* text, int text_bytes) {
  const std::string why =
      abn::sim_observe_refusal(n_rows, node_of_row, (const uint64_t*)othr, n_sites, packed_in, in_stride, packed_out, out_stride);
  put_text(text, text_bytes, why);
  if (!why.empty()) return 1;
  const uint64_t* t = (const uint64_t*)othr;
  if (walk_blocks <= 0) abn::sim_observe_serial(seed, n_rows, node_of_row, t, n_sites, packed_in, in_stride, packed_out, out_stride);
  else if (lazy) abn::sim_observe_walk<true>(seed, n_rows, node_of_row, t, n_sites, walk_blocks, packed_in, in_stride, packed_out, out_stride);
  else abn::sim_observe_walk<false>(seed, n_rows, node_of_row, t, n_sites, walk_blocks, packed_in, in_stride, packed_out, out_stride);
  return 0;
}
// abn_packed_census_windows on the host: counts [n_windows x n_samples x 3].  walk_chunk = 0: field by field; > 0 (a
// multiple of 256): the kernels' job structure walked with that many sites per job
int abn_packed_census_windows_host(const unsigned char* packed, int n_samples, long long n_sites, long long row_stride,
                                   const long long* site_begin, const long long* site_end, int n_windows,
                                   unsigned long long* counts, long long walk_chunk, char* text, int text_bytes) {
  static_assert(sizeof(long long) == sizeof(int64_t), "window ranges");
  std::string why = abn::census_refusal(packed, n_samples, n_sites, row_stride, (const int64_t*)site_begin, (const int64_t*)site_end,
                                        n_windows, counts);
  if (why.empty() && (walk_chunk < 0 || walk_chunk % abn::kPackedStepSites != 0 || walk_chunk >= (1ll << 30)))
    why = "walk_chunk is not a multiple of 256 below 2^30";
  put_text(text, text_bytes, why);
  if (!why.empty()) return 1;
  if (walk_chunk == 0) {
    abn::census_windows_serial(packed, n_samples, row_stride, (const int64_t*)site_begin, (const int64_t*)site_end, n_windows,
                               (uint64_t*)counts);
  } else {
    const std::vector<long long> chunk((size_t)n_windows, walk_chunk);
    abn::census_windows_walk(packed, n_samples, row_stride, (const int64_t*)site_begin, (const int64_t*)site_end, n_windows,
                             chunk.data(), (uint64_t*)counts);
  }
  return 0;
}
// ---- region states (csrc/abn_regions.hpp) in their host forms, for tests/test_regions_cpu.py and test_regions_gpu.py
// abn_packed_region_states on the host: out [n_samples x abn_packed_row_stride(n_columns)].  walk = 0: the law field by
// field; else the kernel's lane and workgroup structure, long windows through the census's walk.  1 with the refusal's
// words in `text`
int abn_packed_region_states_host(const unsigned char* packed, int n_samples, long long n_sites, long long row_stride,
                                  const long long* site_begin, const long long* site_end, long long n_windows, const int* src,
                                  long long n_columns, long long lo_num, long long hi_num, long long den, long long min_kept,
                                  long long long_sites, unsigned char* out, int walk, char* text, int text_bytes) {
  const int64_t* b = (const int64_t*)site_begin;
  const int64_t* e = (const int64_t*)site_end;
  const std::string why = abn::region_refusal(packed, n_samples, n_sites, row_stride, b, e, n_windows, src, n_columns, lo_num,
                                              hi_num, den, min_kept, long_sites, out);
  put_text(text, text_bytes, why);
  if (!why.empty()) return 1;
  const abn::RegionRule rule{(uint64_t)lo_num, (uint64_t)hi_num, (uint64_t)den, (uint64_t)min_kept};
  const long long out_stride = (n_columns + abn::kPackedStepSites - 1) / abn::kPackedStepSites * 64;
  if (walk) abn::region_states_walk(packed, n_samples, row_stride, b, e, n_windows, src, n_columns, rule,
                                    abn::region_long_sites(long_sites), out, out_stride);
  else abn::region_states_serial(packed, n_samples, row_stride, b, e, src, n_columns, rule, out, out_stride);
  return 0;
}
// region_call on planted counts; -1 for a rule outside the law's bounds
int abn_region_call_host(unsigned long long n0, unsigned long long n1, unsigned long long n2, long long lo_num, long long hi_num,
                         long long den, long long min_kept) {
  if (den < 1 || den > (1ll << 20) || lo_num < 0 || lo_num > hi_num || hi_num > den || min_kept < 1) return -1;
  return (int)abn::region_call(n0, n1, n2, abn::RegionRule{(uint64_t)lo_num, (uint64_t)hi_num, (uint64_t)den, (uint64_t)min_kept});
}
}
