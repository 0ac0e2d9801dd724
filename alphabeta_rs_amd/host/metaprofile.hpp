// metaprofile.hpp — the `alphabeta_multiple` half of the reference's `metaprofile` binary
// (src/cli/metaprofile.rs:33-114; SURVEY.md §8f row 2, "next"): the SERIAL window loop that calls
// alphabeta::run once per (region, window) directory becomes ONE batched, device-resident plan
// (abn_plan_*: W windows x (S starts + B bootstraps) in three kernel launches) behind ONE batched pedigree
// construction (Pedigree::build_many -> abn_pairwise_divergence_windows_packed).  That path starts from the directory
// tree the reference's `extract` stage writes: <output_dir>/<region>/<window>/{nodelist,edgelist}.txt and the samples'
// window files (src/setup.rs:35-72, src/windows.rs:259-285).
//
// The `extract` stage itself (src/extract.rs:17-155) is extract_in_memory: whole methylome files and a gene annotation
// in, every site placed into its windows on the device (windows_extract.hpp, abn_windows_*), the packed matrix of the
// scan written there directly — no file tree in between — and alphabeta_multiple_in_memory runs the scan, the fits and the
// analysis on it.  --invert and the "load an existing extraction" shortcut (src/windows.rs:178-243) are not part of it.
//
// Outputs as the reference: results.txt (:74-99, ';'-separated, one line per successful window) and
// raw.npy, the (iterations, 7, n_windows) array of :49,68,110.  The metaplot PNG (:113) is not produced.
#pragma once

#include <filesystem>
#include <iostream>
#include <memory>

#include "alphabeta.hpp"

namespace alphabeta {
namespace metaprofile {

struct WindowArgs {  // the fields of arguments::Windows (src/arguments.rs:6-62) this driver reads
  std::string output_dir = ".";
  std::string name = "Anonymous Run";
  uint32_t window_step = 5;      // 0 means window_size (src/cli/metaprofile.rs:18-20)
  uint32_t window_size = 5;
  uint32_t cutoff = 2048;
  bool absolute = false;
  size_t iterations = 100;
  double posterior_max_filter = 0.99;  // AlphaBeta::default (src/arguments.rs:142-152)
  // extract_in_memory only
  std::string methylome, genome;  // directory of methylome files, annotation file
  std::string nodes, edges;       // the one nodelist / edgelist of every window (arguments::AlphaBeta)
  bool cutoff_gene_length = false;
  bool invert = false;            // refused
  bool device_parse = false;      // --parse device: the methylome files through abn_sites_parse (not in the reference)
  bool device_genes = false;      // --genes device: every site's gene through abn_windows_create_sites (abn_genes_*)
  bool device_sites = false;      // --sites device (with both of the above): the parsed records stay on the device up to
                                  // the window matrix (abn_sites_parse_dev, abn_windows_create_parsed)
  bool sort = false;              // --sort (with --sites device, --tiles or --regions): every methylome is sorted by genomic
                                  // position on the device behind its parse (abn_sites_sort)
  int dedup = -1;                 // --dedup POLICY (where --sort is accepted): an ABN_DEDUP_* policy, -1 none; implies the sort,
                                  // and every run of records with one key is collapsed on the device (abn_sites_dedup)
  Align align = Align::None;      // --align position (with --sites device): only the sites every sample shares are placed
                                  // (abn_windows_create_aligned): no ragged window; the side files describe those sites.
                                  // --align union: every sample gets all the sites any sample holds, filtered
                                  // placeholders where it lacks one (abn_windows_create_union): no ragged window either;
                                  // the side files count union sites
};

struct WindowResult {
  Model model;
  Analysis analysis;
  std::string region;
  double obs_meth_lvl;
  size_t window_index;  // position in the (region, window) enumeration
};

struct Output {
  std::vector<WindowResult> results;
  std::vector<double> raw;  // (iterations, 7, n_ok) C order
  size_t n_ok = 0, iterations = 0;
  std::string results_txt;
};

struct Win {  // a window whose pedigree was built
  std::string region;
  Pedigree ped;
  double p0uu;
  size_t index;  // position in the (region, window) enumeration
};
inline Output fit_windows(const WindowArgs& args, std::vector<Win> wins, const std::vector<int>& distribution);

// results.txt (src/cli/metaprofile.rs:74-96): the header, and one window's line
inline std::string results_header() {
  return "run;window;cg_count;region;alpha;beta;1/2*(alpha+beta);pred_steady_state;obs_steady_state;sd_alpha;sd_beta;"
         "ci_alpha_0.025;ci_alpha_0.975;ci_beta_0.025;ci_beta_0.975\n";
}
inline std::string results_line(const std::string& name, size_t window, long long cg_count, const WindowResult& r) {
  const Model& m = r.model;
  const Analysis& a = r.analysis;
  return name + ";" + std::to_string(window) + ";" + std::to_string(cg_count) + ";" + r.region + ";" + fmt_f64(m.alpha) +
         ";" + fmt_f64(m.beta) + ";" + fmt_f64(0.5 * (m.alpha + m.beta)) + ";" + fmt_f64(steady_state(m.alpha, m.beta)) + ";" +
         fmt_f64(r.obs_meth_lvl) + ";" + fmt_f64(a.sd_alpha) + ";" + fmt_f64(a.sd_beta) + ";" + fmt_f64(a.ci_alpha.lo) + ";" +
         fmt_f64(a.ci_alpha.hi) + ";" + fmt_f64(a.ci_beta.lo) + ";" + fmt_f64(a.ci_beta.hi) + "\n";
}

inline uint32_t window_step(const WindowArgs& args) {  // src/cli/metaprofile.rs:18-20, src/extract.rs:26-28
  return args.window_step == 0 ? args.window_size : args.window_step;
}

// The (region, window) enumeration of src/cli/metaprofile.rs:34-53, in its order: `window` = 0, step, .. below the region's
// max.  It names ceil(max / step) windows per region where Windows::new (src/windows.rs:28-44) creates floor(max / step):
// created = this one exists, and then w is its place among the created ones (upstream, gene, downstream).
struct NamedWindow {
  std::string region;
  uint32_t window;
  bool created;
  size_t w;
};
inline std::vector<NamedWindow> enumerate_windows(const WindowArgs& args, uint32_t max_gene_length) {
  const uint32_t step = window_step(args);
  const std::pair<const char*, uint32_t> regions[3] = {{"upstream", args.cutoff}, {"gene", max_gene_length}, {"downstream", args.cutoff}};
  std::vector<NamedWindow> out;
  size_t first = 0;
  for (const auto& region : regions) {
    const uint32_t max = args.absolute ? region.second : 100, count = step ? max / step : 0;
    for (uint32_t window = 0, k = 0; window < max; window += step, ++k)
      out.push_back(NamedWindow{region.first, window, k < count, first + k});
    first += count;
  }
  return out;
}

// src/cli/metaprofile.rs:33-114
inline Output alphabeta_multiple(const WindowArgs& args, uint32_t max_gene_length, const std::vector<int>& distribution) {
  namespace fs = std::filesystem;
  std::vector<Win> wins;
  // every (region, window) directory in the reference's order; all pedigrees are built together (Pedigree::build_many:
  // one batched pairwise scan instead of one per window), then reported in that order, each window's diagnostics first
  std::vector<std::pair<std::string, std::string>> lists;
  std::vector<std::string> region_of;
  for (const NamedWindow& nw : enumerate_windows(args, max_gene_length)) {
    const fs::path dir = fs::path(args.output_dir) / nw.region / std::to_string(nw.window);
    lists.push_back({(dir / "nodelist.txt").string(), (dir / "edgelist.txt").string()});
    region_of.push_back(nw.region);
  }
  std::vector<Pedigree::Built> built = Pedigree::build_many(lists, args.posterior_max_filter, /*gpu_pairwise=*/true, args.device_parse);
  for (size_t index = 0; index < built.size(); ++index) {
    Pedigree::Built& b = built[index];
    std::fputs(b.diagnostics.c_str(), stdout);  // where the per-window build printed them: before the window's outcome
    // alphabeta::run's pedigree build; a failing window is reported and skipped (:64-65)
    if (b.ok && b.pedigree.nrows() == 0) b.ok = false, b.error = "empty pedigree";
    if (b.ok)
      wins.push_back(Win{region_of[index], std::move(b.pedigree), b.p0uu, index});
    else
      std::printf("Error: Error while building pedigree: %s\n", b.error.c_str());
  }
  return fit_windows(args, std::move(wins), distribution);
}

// The windows' fits, analyses and results.txt (src/cli/metaprofile.rs:50-110 behind the pedigree build)
inline Output fit_windows(const WindowArgs& args, std::vector<Win> wins, const std::vector<int>& distribution) {
  Output out;
  out.iterations = args.iterations;
  if (wins.empty()) return out;

  // Windows that share the (t0, t1, t2) rows (the normal case: one nodelist/edgelist for all windows) are
  // fitted by one plan; anything else gets a plan of its own.
  auto same_topology = [](const Pedigree& a, const Pedigree& b) {
    if (a.nrows() != b.nrows()) return false;
    for (size_t i = 0; i < a.nrows(); ++i)
      for (size_t c = 0; c < 3; ++c)
        if (a.at(i, c) != b.at(i, c)) return false;
    return true;
  };
  std::vector<int> group(wins.size(), -1);
  int ngroups = 0;
  for (size_t i = 0; i < wins.size(); ++i) {
    if (group[i] >= 0) continue;
    group[i] = ngroups;
    for (size_t j = i + 1; j < wins.size(); ++j)
      if (group[j] < 0 && same_topology(wins[i].ped, wins[j].ped)) group[j] = ngroups;
    ++ngroups;
  }
  Device& dev = default_device();
  const size_t B = args.iterations, S = args.iterations;  // n_starts = n_boot = iterations (src/alphabeta.rs:33-54)
  std::vector<Model> models(wins.size());
  std::vector<RawAnalysis> raws(wins.size());
  std::vector<char> ok(wins.size(), 0);
  for (int g = 0; g < ngroups; ++g) {
    std::vector<size_t> members;
    for (size_t i = 0; i < wins.size(); ++i)
      if (group[i] == g) members.push_back(i);
    const Pedigree& p0 = wins[members[0]].ped;
    const size_t N = p0.nrows(), W = members.size();
    std::vector<double> gens(N * 3), D(W * N), p0uu(W);
    for (size_t i = 0; i < N; ++i)
      for (size_t c = 0; c < 3; ++c) gens[i * 3 + c] = p0.at(i, c);
    for (size_t w = 0; w < W; ++w) {
      for (size_t i = 0; i < N; ++i) D[w * N + i] = wins[members[w]].ped.at(i, 3);
      p0uu[w] = wins[members[w]].p0uu;
    }
    // every window draws from the Philox streams of ITS position in the (region, window) enumeration, whatever
    // windows failed before it and whichever topology group it landed in
    std::vector<uint32_t> ids(W);
    for (size_t w = 0; w < W; ++w) ids[w] = (uint32_t)wins[members[w]].index;
    std::vector<double> mod(W * 4), raw(W * B * 7);
    std::vector<int32_t> best(W);
    // one plan per device (abn_multi_*: --devices; one device = one plan), windows in contiguous blocks, the bootstrap
    // tables gathered with RCCL: the loop of src/cli/metaprofile.rs:50-72 in three launches per device
    std::vector<int32_t> devs = device_list();
    if (devs.empty()) devs.push_back(0);
    {
      MultiDevice md(devs, dev.options, gens.data(), N, W, S, B);
      md.check(abn_multi_set_window_ids(md.get(), ids.data()), "abn_multi_set_window_ids");
      if (dev.stream_sweep) md.check(abn_multi_set_stream_sweep(md.get(), 1), "abn_multi_set_stream_sweep");
      md.check(abn_multi_set_windows(md.get(), D.data(), p0uu.data(), nullptr, nullptr), "abn_multi_set_windows");
      md.check(abn_multi_run(md.get()), "abn_multi_run");
      int rc = abn_multi_download(md.get(), mod.data(), nullptr, nullptr, raw.data(), nullptr, nullptr, best.data());
      if (rc == ABN_ERR_NO_FINITE_FIT) rc = ABN_OK;  // per window below: best[w] < 0 is printed and skipped (:64-65)
      md.check(rc, "metaprofile plan");
    }
    for (size_t w = 0; w < W; ++w) {
      const size_t i = members[w];
      if (best[w] < 0) {
        std::printf("Error: Model failed: %s\n", abn_status_string(ABN_ERR_NO_FINITE_FIT));
        continue;
      }
      models[i] = Model::from_ptr(&mod[w * 4]);
      raws[i].n_boot = B;
      raws[i].rows.assign(raw.begin() + (std::ptrdiff_t)(w * B * 7), raw.begin() + (std::ptrdiff_t)((w + 1) * B * 7));
      ok[i] = 1;
    }
  }
  for (size_t i = 0; i < wins.size(); ++i) {
    if (!ok[i]) continue;
    try {
      out.results.push_back(WindowResult{models[i], raws[i].analyze(), wins[i].region, 1.0 - wins[i].p0uu, wins[i].index});
    } catch (const Error& e) {  // a bootstrap table with non-finite fits: this window fails, the others go on (:64-65)
      std::printf("Error: Model failed: %s\n", e.what());
      ok[i] = 0;
    }
  }
  out.n_ok = out.results.size();
  // raw_analyses.push(Axis(2), ...) -> (iterations, 7, n_ok), C order (:49,68)
  out.raw.assign(B * 7 * out.n_ok, 0.0);
  {
    size_t k = 0;
    for (size_t i = 0; i < wins.size(); ++i) {
      if (!ok[i]) continue;
      for (size_t b = 0; b < B; ++b)
        for (size_t c = 0; c < 7; ++c) out.raw[(b * 7 + c) * out.n_ok + k] = raws[i].rows[b * 7 + c];
      ++k;
    }
  }
  // :74-96 — results zipped with `distribution`: the shorter of the two decides the number of lines
  std::string print = results_header();
  const size_t nl = std::min(out.results.size(), distribution.size());
  for (size_t i = 0; i < nl; ++i) print += results_line(args.name, i, distribution[i], out.results[i]);
  out.results_txt = print;
  return out;
}

// ------------------------------------------------------------------------------------------------
// The `extract` stage without the file tree (src/extract.rs:17-155)
struct Extraction {
  std::vector<std::string> names;           // the methylome files, sorted by name (the reference takes read_dir's order)
  std::unique_ptr<windows::Handle> handle;  // every sample's sites placed, packed and summed, device-resident
  abn_windows_params params{};
  uint32_t max_gene_length = 100;
  std::vector<int> distribution;  // the first methylome's window counts (src/extract.rs:154)
};

// src/extract.rs:17-155: parse the annotation and every methylome once, choose every site's gene (on the host, or with
// device_genes on the device; with device_sites the parsed records never leave it), place the sites into windows on the
// device; write distribution_<name>, distributions.txt, steady_state_methylation.txt and
// all_steady_state_methylation.txt (:112-151, src/windows.rs:130-176,245-257) into the output directory.
inline Extraction extract_in_memory(const WindowArgs& args) {
  namespace fs = std::filesystem;
  if (args.invert) throw Error(ABN_ERR_INVALID_ARG, "--invert is not supported with --methylome");
  const uint32_t step = window_step(args);
  if (step == 0) throw Error(ABN_ERR_INVALID_ARG, "window step and window size are both 0");
  Extraction ex;
  // files::load_methylome (src/files.rs:23-38): files with an extension other than *tsv* / *fn*
  {
    std::error_code ec;
    fs::directory_iterator it(args.methylome, ec);
    if (ec) throw Error(ABN_ERR_INVALID_ARG, "could not read the methylome directory " + args.methylome);
    for (const auto& e : it) {
      const std::string ext = e.path().extension().string();
      if (ext.empty() || ext.find("tsv") != std::string::npos || ext.find("fn") != std::string::npos) continue;
      if (!e.is_regular_file()) continue;
      ex.names.push_back(e.path().filename().string());
    }
    std::sort(ex.names.begin(), ex.names.end());
  }
  if (ex.names.empty())
    throw Error(ABN_ERR_INVALID_ARG, "Could not find any files in the methylome directory. Please check your input. "
                                     "Files with .tsv or .fn extensions are ignored.");
  std::string annotation;
  try {
    annotation = detail::read_file(args.genome, "annotation");
  } catch (const Error&) {
    throw Error(ABN_ERR_INVALID_ARG, "Error while reading genome annotation file: " + args.genome);
  }
  const windows::Genome genome = windows::parse_annotation(annotation);
  if (genome.n_genes == 0)
    throw Error(ABN_ERR_INVALID_ARG, "Could not parse a single annotation from the annotation file. Please check your "
                                     "input or add a parser implemenation for your data format.");
  if (args.absolute) {
    ex.max_gene_length = genome.max_gene_length;
    std::printf("The maximum gene length is %u bp\n", ex.max_gene_length);
  }
  ex.params = windows::window_params(args.cutoff, step, args.window_size, args.absolute, ex.max_gene_length);
  if (args.device_sites && !(args.device_parse && args.device_genes))
    throw Error(ABN_ERR_INVALID_ARG, "--sites device needs --parse device and --genes device");
  if (args.align != Align::None && !args.device_sites)
    throw Error(ABN_ERR_INVALID_ARG, std::string("--align ") + align_name(args.align) + " needs --sites device");
  if (args.sort && !args.device_sites) throw Error(ABN_ERR_INVALID_ARG, "--sort needs --sites device");
  if (args.dedup >= 0 && !args.device_sites) throw Error(ABN_ERR_INVALID_ARG, "--dedup needs --sites device");
  if (args.device_sites) {
    // every text goes up, its records stay there; it is dropped as soon as its deferred lines are decided
    const windows::GeneRule rule{args.cutoff, args.cutoff_gene_length};
    resident::Samples samples{default_device(), /*skip_lines=*/1, {}, 1u, args.sort, args.dedup};
    for (const auto& name : ex.names) samples.add_text(detail::read_file((fs::path(args.methylome) / name).string(), "methylome"), name);
    for (const std::string& line : samples.sort_report) std::fputs(line.c_str(), stdout);
    ex.handle = std::make_unique<windows::Handle>(default_device(), ex.params, genome, rule, args.posterior_max_filter,
                                                  samples.sites, args.align);
    for (const std::string& line : resident::align_report(args.align, ex.names, resident::align_counts(*ex.handle, args.align)))
      std::fputs(line.c_str(), stdout);
  } else {
    std::vector<std::string> texts;
    for (const auto& name : ex.names) texts.push_back(detail::read_file((fs::path(args.methylome) / name).string(), "methylome"));
    const windows::GeneRule rule{args.cutoff, args.cutoff_gene_length};
    if (args.device_genes) {
      // the parsed sites (with --parse device: the merged sequence, deferred lines decided here) go up once; the gene of
      // every site is chosen there
      const auto sites = windows::parse_sites_many(texts, args.device_parse ? &default_device() : nullptr);
      std::vector<std::string>().swap(texts);
      ex.handle = std::make_unique<windows::Handle>(default_device(), ex.params, genome, rule, args.posterior_max_filter, sites);
    } else {
      const std::vector<windows::SampleSites> samples =
          args.device_parse
              ? windows::choose_genes_many_device(default_device(), texts, genome, rule, args.posterior_max_filter)
              : windows::choose_genes_many(texts, genome, rule, args.posterior_max_filter);
      ex.handle = std::make_unique<windows::Handle>(default_device(), ex.params, samples);
    }
  }
  const windows::Handle& h = *ex.handle;
  const size_t n = h.n_samples(), W = h.n_windows();
  for (size_t w = 0; w < W; ++w) ex.distribution.push_back((int)h.count[w]);
  // the four kinds of side files
  std::string all_dist, all_meth, avg_txt;
  std::vector<double> average(W, 0.0);
  for (size_t s = 0; s < n; ++s) {
    std::string dist;
    all_dist += ex.names[s] + ";";
    all_meth += ex.names[s] + ";";
    for (size_t w = 0; w < W; ++w) {
      const long long cnt = (long long)h.count[s * W + w];
      const double m = h.level_sum[s * W + w] / (double)cnt;  // fold / len, NaN for an empty window (:112)
      dist += std::to_string((int)cnt) + "\n";
      all_dist += std::to_string((int)cnt) + ";";
      all_meth += fmt_f64(m) + ";";
      average[w] += m / (double)n;  // src/extract.rs:106-110
    }
    all_dist += "\n";
    all_meth += "\n";
    std::ofstream(fs::path(args.output_dir) / ("distribution_" + ex.names[s]), std::ios::binary) << dist;
  }
  for (size_t w = 0; w < W; ++w) avg_txt += fmt_f64(average[w]) + "\n";
  std::ofstream(fs::path(args.output_dir) / "steady_state_methylation.txt", std::ios::binary) << avg_txt;
  std::ofstream(fs::path(args.output_dir) / "all_steady_state_methylation.txt", std::ios::binary) << all_meth;
  std::ofstream(fs::path(args.output_dir) / "distributions.txt", std::ios::binary) << all_dist;
  return ex;
}

// One window's (or tile's) pedigree from what a handle reports: level_sum_kept and kept [n_samples x n_windows], and dv,
// window w's D values for the n_samples * (n_samples - 1) / 2 pairs of samples in the scan's order.  sample_of: the sample
// of every sampled node; times: detail::convert_times of the graph.  p0uu as src/pedigree.rs:165-166,180-184 folds it.
// Two nodes that name one sample have no pair in the scan: their D is 0, or NaN when the sample kept no site.
inline Win window_from_handle(const std::string& region, size_t index, const std::vector<detail::PairTimes>& times,
                              const std::vector<size_t>& sample_of, size_t n_samples, size_t n_windows, size_t w,
                              const std::vector<double>& level_sum_kept, const std::vector<int64_t>& kept, const double* dv) {
  const size_t nn = sample_of.size(), n = n_samples, W = n_windows;
  std::vector<double> dm(nn * nn, 0.0);
  double p0 = 0.0;
  for (size_t a = 0; a < nn; ++a) {
    const size_t sa = sample_of[a];
    p0 += 1.0 - level_sum_kept[sa * W + w] / (double)kept[sa * W + w];
    for (size_t b = a + 1; b < nn; ++b) {
      const size_t sb = sample_of[b], i = std::min(sa, sb), j = std::max(sa, sb);
      dm[a * nn + (b - a - 1)] = i == j ? (kept[sa * W + w] > 0 ? 0.0 : std::nan("")) : dv[i * n - i * (i + 1) / 2 + (j - i - 1)];
    }
  }
  Pedigree ped = detail::rows_from(times, dm, nn);
  if (ped.nrows() == 0) throw Error(ABN_ERR_BAD_PEDIGREE, "empty pedigree");
  return Win{region, std::move(ped), p0 / (double)nn, index};
}

// alphabeta_multiple (src/cli/metaprofile.rs:33-114) on an Extraction: the pedigrees and p0uu come from the handle — one
// scan of the resident matrix for all windows, detail::convert_times once for the graph they share — instead of
// Pedigree::build_many on window directories.  Window ids stay the position in the enumeration (enumerate_windows): the
// window it names beyond those created fails as its missing sample file fails there.  A RAGGED window (the samples' site
// counts differ) fails too; the reference goes on with D = 0 for its pairs (DESIGN.md §4 "Window placement").  With
// args.align the handle holds only the sites every sample shares, or every sample the union of all sites, so no window is
// ragged.  A graph DMatrix::convert refuses is reported at every window that gets as far as the conversion — each window
// is a run of the reference's, which fails there — and the run goes on to its empty result.
inline Output alphabeta_multiple_in_memory(const WindowArgs& args, const Extraction& ex) {
  namespace fs = std::filesystem;
  const windows::Handle& h = *ex.handle;
  const size_t n = h.n_samples(), W = h.n_windows(), npairs = n * (n - 1) / 2;
  const detail::Inputs graph = detail::read_graph(args.nodes, args.edges);
  const size_t nn = graph.nodes.size();
  std::vector<size_t> sample_of(nn);
  for (size_t i = 0; i < nn; ++i) {
    const auto it = std::find(ex.names.begin(), ex.names.end(), resident::base_name(graph.nodes[i].file));
    if (it == ex.names.end()) throw Error(ABN_ERR_INVALID_ARG, "Could not open node file: " + graph.nodes[i].file);
    sample_of[i] = (size_t)(it - ex.names.begin());
  }
  std::vector<double> dv(std::max<size_t>(W * npairs, 1), 0.0);
  default_device().check(abn_windows_pairwise(h.get(), nullptr, nullptr, dv.data()), "abn_windows_pairwise");
  std::vector<detail::PairTimes> times;
  std::unique_ptr<Error> graph_refused;  // what convert throws from the graph alone
  try {
    times = detail::convert_times(graph);
  } catch (const Error& e) {
    graph_refused = std::make_unique<Error>(e);
  }
  std::vector<Win> wins;
  const std::vector<NamedWindow> named = enumerate_windows(args, ex.max_gene_length);
  for (size_t index = 0; index < named.size(); ++index) {
    const NamedWindow& nw = named[index];
    try {
      if (!nw.created)  // no sample file in that directory
        throw Error(ABN_ERR_INVALID_ARG,
                    "Could not open node file: " + (fs::path(args.output_dir) / nw.region / std::to_string(nw.window) /
                                                    (nn ? resident::base_name(graph.nodes[0].file) : std::string()))
                                                       .string());
      const size_t w = nw.w;
      if (h.ragged[w]) {
        for (size_t a = 0; a < nn; ++a)
          for (size_t b = a + 1; b < nn; ++b)
            if (h.count[sample_of[a] * W + w] != h.count[sample_of[b] * W + w])
              std::printf("Lengths do not match, all bets are off: %zu vs %zu\n", (size_t)h.count[sample_of[a] * W + w],
                          (size_t)h.count[sample_of[b] * W + w]);
        throw Error(ABN_ERR_INVALID_ARG, "the samples' site counts differ in this window");
      }
      if (graph_refused) throw *graph_refused;
      wins.push_back(window_from_handle(nw.region, index, times, sample_of, n, W, w, h.level_sum_kept, h.kept, &dv[w * npairs]));
    } catch (const std::exception& e) {
      std::printf("Error: Error while building pedigree: %s\n", e.what());
    }
  }
  return fit_windows(args, std::move(wins), ex.distribution);
}

// ndarray_npy::write_npy of the (iterations, 7, n_windows) array (:110)
inline void write_raw_npy(const Output& o, const std::string& path) {
  std::string dict = "{'descr': '<f8', 'fortran_order': False, 'shape': (" + std::to_string(o.iterations) + ", 7, " +
                     std::to_string(o.n_ok) + "), }";
  const size_t total = 10 + dict.size() + 1;
  dict += std::string((64 - total % 64) % 64, ' ') + "\n";
  std::ofstream f(path, std::ios::binary);
  const char magic[8] = {'\x93', 'N', 'U', 'M', 'P', 'Y', 1, 0};
  f.write(magic, 8);
  const uint16_t hl = (uint16_t)dict.size();
  f.write(reinterpret_cast<const char*>(&hl), 2);
  f.write(dict.data(), (std::streamsize)dict.size());
  f.write(reinterpret_cast<const char*>(o.raw.data()), (std::streamsize)(o.raw.size() * sizeof(double)));
}

}  // namespace metaprofile
}  // namespace alphabeta
