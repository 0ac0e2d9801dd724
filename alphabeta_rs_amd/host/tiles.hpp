// tiles.hpp — epimutation rates per GENOMIC TILE: the batched metaprofile fit (metaprofile.hpp: fit_windows) over fixed bins
// of the genome (--tiles SIZE [--tile-step STEP]) or the rows of a region list (--regions FILE: a BED-like file of TEs,
// promoters, chromatin states — the 4-column rows src/methylation_site.rs parses anticipate such lists), where the
// reference asks one pedigree for the whole genome (src/cli/alphabeta.rs) or gene-relative windows
// (src/cli/metaprofile.rs:33-114).  Every methylome is parsed on the device and stays there (abn_sites_parse_dev);
// abn_tiles_* (csrc/abn_tiles.hpp) aligns them, finds every tile's columns and folds rc_meth_lvl per (sample, tile); one
// scan gives every tile's D matrix; every tile is then a window of fit_windows, its Philox streams those of its index in
// the tile list.  No annotation, no file tree.  With --pool the rows of the list that share a name are one POOL
// (abn_tiles_set_pools): one pedigree from every site inside any of them — one rate per annotation class — and from there
// on a tile like the others.
#pragma once

#include <unordered_map>

#include "block_bootstrap.hpp"
#include "metaprofile.hpp"
#include "region_states.hpp"

namespace alphabeta {
namespace metaprofile {

struct TileArgs {
  int64_t size = 0, step = 0;  // --tiles SIZE [--tile-step STEP]: fixed tiles (step 0: size)
  std::string regions;         // --regions FILE: a list
  bool pool = false;           // --pool: the rows of the list that share a name are one pool, one pedigree (region_pools)
  int64_t block_replicates = 0;  // --block-bootstrap R (0: none) and --block-starts S (block_bootstrap.hpp)
  int block_starts = kBlockStartsDefault;
  RegionArgs region;             // --region-states LO,HI [--region-min-sites K] (region_states.hpp)
  bool fixed() const { return regions.empty(); }
};

struct TileList {
  std::vector<int32_t> chromosome;  // Numbered(n) = n, Mitochondrial = 256, Chloroplast = 257
  std::vector<int64_t> start, end;
  std::vector<std::string> name;    // the row's 4th field; empty: the row has three
  size_t size() const { return chromosome.size(); }
};

// a tile bound: decimal digits, at most 2^32
inline bool parse_tile_bound(const std::string& t, int64_t& v) {
  if (t.empty() || t.size() > 10) return false;
  int64_t acc = 0;
  for (char ch : t) {
    if (ch < '0' || ch > '9') return false;
    acc = acc * 10 + (ch - '0');
  }
  if (acc > (int64_t)1 << 32) return false;
  v = acc;
  return true;
}

// A BED-like region list: fields split at tab or space, the first three are chromosome, start, end; the chromosome is
// spelled as in a methylome (src/methylation_site.rs:55-68: `chr` stripped, M, C, a number up to 255).  A line that does
// not parse (a header, `track`, `#`) is skipped; the tiles keep the file's order.
inline TileList read_regions(const std::string& text) {
  TileList out;
  for (std::string line : detail::split_any(text, "\n")) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    std::vector<std::string> f;
    for (const std::string& t : detail::split_any(line, "\t "))
      if (!t.empty()) f.push_back(t);
    int key;
    int64_t a, b;
    if (f.size() < 3 || !windows::parse_chromosome_key(f[0], key) || !parse_tile_bound(f[1], a) || !parse_tile_bound(f[2], b))
      continue;
    out.chromosome.push_back(key);
    out.start.push_back(a);
    out.end.push_back(b);
    out.name.push_back(f.size() > 3 ? f[3] : std::string());
  }
  return out;
}

// --pool: the rows of a region list by name — all genes, all TEs, each chromatin state.  The pools are numbered by first
// appearance in the file; a row without a name (fewer than four fields) is skipped and counted; a name that holds the `;`
// of results.txt and pools.txt is refused.
struct RegionPools {
  TileList rows;                   // the named rows, in file order
  std::vector<int32_t> pool;       // [rows] the row's pool
  std::vector<std::string> names;  // [n_pools]
  std::vector<int64_t> intervals;  // [n_pools] the pool's rows
  size_t skipped = 0;
  std::string refused;             // not empty: why the list is not taken
};
inline RegionPools region_pools(const TileList& list) {
  RegionPools out;
  std::unordered_map<std::string, int32_t> seen;
  for (size_t k = 0; k < list.size(); ++k) {
    const std::string& name = list.name[k];
    if (name.empty()) {
      ++out.skipped;
      continue;
    }
    if (name.find(';') != std::string::npos) {
      out.refused = "region " + std::to_string(k) + ": the name '" + name + "' holds a ';', the separator of the output files";
      return out;
    }
    const auto at = seen.emplace(name, (int32_t)out.names.size());
    if (at.second) out.names.push_back(name), out.intervals.push_back(0);
    ++out.intervals[(size_t)at.first->second];
    out.rows.chromosome.push_back(list.chromosome[k]);
    out.rows.start.push_back(list.start[k]);
    out.rows.end.push_back(list.end[k]);
    out.rows.name.push_back(name);
    out.pool.push_back(at.first->second);
  }
  return out;
}

inline std::string chromosome_name(int32_t c) { return c == 256 ? "M" : (c == 257 ? "C" : std::to_string(c)); }
inline std::string tile_region(int32_t c, int64_t start, int64_t end) {
  return chromosome_name(c) + ":" + std::to_string(start) + "-" + std::to_string(end);
}

struct TilesOutput {
  Output out;             // results_txt: `window` = the tile's index in the list, `cg_count` = the tile's columns
  std::string tiles_txt;  // tile;chromosome;start;end;cg_count;fitted, every tile of the list
  std::string pools_txt;  // --pool, in its place: pool;name;intervals;segments;cg_count;fitted, every pool
  transitions::Table transitions;  // --transitions: the table of every tile (pool), fitted or not, in the rows' order
  BlockBootstrap block;            // --block-bootstrap: block_bootstrap.txt and block_raw.npy
  // --region-states, in place of tiles.txt / pools.txt: regions.txt (column;tile;chromosome;start;end;cg_count;group, every
  // column of the region matrix), groups.txt (--pool: group;name;regions;fitted) and region_states.npy (uint8, samples x
  // columns: the called fields, rows in the nodes' order)
  std::string regions_txt, groups_txt;
  std::vector<uint8_t> region_states;
  size_t region_rows = 0, region_columns = 0;
};

// The sibling of alphabeta_multiple_in_memory for tiles.  args: methylome (directory), nodes, edges, align, iterations,
// posterior_max_filter, name.  A tile without a column, with a sampled node that has no counted site, or with a sampled
// pair that shares no compared site is reported and skipped; the others go on (src/cli/metaprofile.rs:64-65).  A graph
// DMatrix::convert refuses ends the run.
// The sampled nodes of a tile run and their methylomes: every line read (src/pedigree.rs:147-163) under the context mask,
// the records left on the device
struct TileSamples {
  detail::Inputs graph;
  std::vector<std::string> names;  // the methylome files' base names, in the nodes' order
  std::vector<size_t> sample_of;
  resident::Samples samples;
};
inline TileSamples load_tile_samples(const WindowArgs& args, unsigned contexts) {
  namespace fs = std::filesystem;
  TileSamples s{detail::read_graph(args.nodes, args.edges), {}, {}, resident::Samples{default_device(), /*skip_lines=*/0, {}, contexts, args.sort, args.dedup}};
  if (s.graph.nodes.empty()) throw Error(ABN_ERR_INVALID_ARG, "the nodelist names no sampled node");
  for (const auto& node : s.graph.nodes) {
    s.sample_of.push_back(s.names.size());
    s.names.push_back(resident::base_name(node.file));
    s.samples.add_file((fs::path(args.methylome) / s.names.back()).string(), s.names.back());
  }
  for (const std::string& line : s.samples.sort_report) std::fputs(line.c_str(), stdout);
  return s;
}

// --region-states behind the tiles: th's tiles (fixed bins or the rows of `list`) become the columns of a region matrix
// (abn_tiles_region_states), grouped by `group` (null: one group, "regions"); every group is then a window of fit_windows
// as a tile is, its level fold the census of the regions' states (sum = n1 / 2 + n2 over kept = n0 + n1 + n2: exact
// doubles, whatever the order of addition), its D the scan of the region matrix over the group's columns.  count [T]: the
// tiles' sites.  results.txt: `window` = the group's index, `cg_count` = its regions.
inline TilesOutput regions_of_tiles(const WindowArgs& args, const TileArgs& tiles, const TileSamples& loaded, abn_tiles* th,
                                    const TileList& list, const std::vector<int64_t>& count, const int32_t* group,
                                    const std::vector<std::string>& group_names) {
  Device& dev = default_device();
  const detail::Inputs& graph = loaded.graph;
  const std::vector<std::string>& names = loaded.names;
  const size_t nn = graph.nodes.size(), npairs = nn * (nn - 1) / 2, G = group_names.size();
  Owned<abn_regions, abn_regions_destroy> rh;
  dev.check(abn_tiles_region_states(th, tiles.region.lo_num, tiles.region.hi_num, kRegionDen, tiles.region.min_sites, group,
                                    (int32_t)G, rh.out()),
            "abn_tiles_region_states");
  int64_t C = 0, stride = 0;
  dev.check(abn_regions_info(rh.get(), nullptr, &C, &stride, nullptr), "abn_regions_info");
  std::vector<int64_t> gb(G), ge(G);
  std::vector<int32_t> src((size_t)C);
  std::vector<uint8_t> packed(nn * (size_t)stride);
  std::vector<uint64_t> census(G * nn * 3, 0), both(std::max<size_t>(G * npairs, 1), 0);
  std::vector<double> dv(std::max<size_t>(G * npairs, 1), 0.0);
  dev.check(abn_regions_layout(rh.get(), gb.data(), ge.data()), "abn_regions_layout");
  dev.check(abn_regions_order(rh.get(), src.data()), "abn_regions_order");
  dev.check(abn_regions_packed(rh.get(), packed.data()), "abn_regions_packed");
  dev.check(abn_regions_census(rh.get(), census.data()), "abn_regions_census");
  dev.check(abn_regions_pairwise(rh.get(), nullptr, both.data(), dv.data()), "abn_regions_pairwise");
  std::printf("Called %lld regions in %zu group%s\n", (long long)C, G, G == 1 ? "" : "s");

  TilesOutput res;
  if (transitions::request().wanted) {
    for (const auto& node : graph.nodes) {
      res.transitions.names.push_back(node.name);
      res.transitions.generations.push_back(node.generation);
    }
    res.transitions.counts.assign(G * npairs * 9, 0);
    if (npairs > 0) dev.check(abn_regions_transitions(rh.get(), res.transitions.counts.data()), "abn_regions_transitions");
  }
  std::vector<double> sum(nn * G);
  std::vector<int64_t> kept(nn * G);
  for (size_t g = 0; g < G; ++g)
    for (size_t a = 0; a < nn; ++a) {
      const uint64_t* k = &census[(g * nn + a) * 3];
      sum[a * G + g] = 0.5 * (double)k[1] + (double)k[2];
      kept[a * G + g] = (int64_t)(k[0] + k[1] + k[2]);
    }
  const std::vector<detail::PairTimes> times = detail::convert_times(graph);
  std::vector<Win> wins;
  for (size_t g = 0; g < G; ++g) {
    try {
      if (ge[g] == gb[g]) throw Error(ABN_ERR_INVALID_ARG, "no region lies in this group");
      for (size_t a = 0; a < nn; ++a)
        if (kept[a * G + g] == 0) throw Error(ABN_ERR_INVALID_ARG, names[a] + " calls no region in this group");
      for (size_t a = 0, p = 0; a < nn; ++a)
        for (size_t b = a + 1; b < nn; ++b, ++p)
          if (both[g * npairs + p] == 0)
            throw Error(ABN_ERR_INVALID_ARG, names[a] + " and " + names[b] + " share no called region in this group");
      wins.push_back(window_from_handle(group_names[g], g, times, loaded.sample_of, nn, G, g, sum, kept, &dv[g * npairs]));
    } catch (const std::exception& e) {
      std::printf("Error: Error while building pedigree: group %zu (%s): %s\n", g, group_names[g].c_str(), e.what());
    }
  }
  res.out = fit_windows(args, std::move(wins), std::vector<int>());
  std::vector<char> fitted(G, 0);
  res.out.results_txt = results_header();
  for (const WindowResult& r : res.out.results) {
    fitted[r.window_index] = 1;
    res.out.results_txt += results_line(args.name, r.window_index, (long long)(ge[r.window_index] - gb[r.window_index]), r);
  }
  res.regions_txt = "column;tile;chromosome;start;end;cg_count;group\n";
  for (size_t g = 0; g < G; ++g)
    for (int64_t c = gb[g]; c < ge[g]; ++c) {
      const size_t t = (size_t)src[(size_t)c];
      res.regions_txt += std::to_string(c) + ";" + std::to_string(t) + ";" + chromosome_name(list.chromosome[t]) + ";" +
                         std::to_string(list.start[t]) + ";" + std::to_string(list.end[t]) + ";" + std::to_string(count[t]) + ";" +
                         std::to_string(g) + "\n";
    }
  if (tiles.pool) {
    res.groups_txt = "group;name;regions;fitted\n";
    for (size_t g = 0; g < G; ++g)
      res.groups_txt += std::to_string(g) + ";" + group_names[g] + ";" + std::to_string(ge[g] - gb[g]) + ";" + (fitted[g] ? "1" : "0") + "\n";
  }
  res.region_rows = nn, res.region_columns = (size_t)C;
  res.region_states.resize(nn * (size_t)C);
  for (size_t a = 0; a < nn; ++a) {
    const uint8_t* row = packed.data() + loaded.sample_of[a] * (size_t)stride;
    for (size_t c = 0; c < (size_t)C; ++c)
      res.region_states[a * (size_t)C + c] = (uint8_t)((row[(c >> 4) * 4 + (c & 3)] >> (2 * ((c >> 2) & 3))) & 3);
  }
  return res;
}

// alphabeta_multiple_tiles behind the loader: sites[i] = sampled node i's methylome
inline TilesOutput tiles_of_samples(const WindowArgs& args, const TileArgs& tiles, const TileSamples& loaded,
                                    const std::vector<windows::ResidentSites>& sites) {
  Device& dev = default_device();
  const detail::Inputs& graph = loaded.graph;
  const std::vector<std::string>& names = loaded.names;
  const std::vector<size_t>& sample_of = loaded.sample_of;
  const size_t nn = graph.nodes.size(), npairs = nn * (nn - 1) / 2;
  TileList list;
  RegionPools pools;
  if (!tiles.fixed()) {
    list = read_regions(detail::read_file(tiles.regions, "regions"));
    if (list.size() == 0) throw Error(ABN_ERR_INVALID_ARG, "Could not parse a single region from " + tiles.regions);
  }
  if (tiles.pool) {
    pools = region_pools(list);
    if (!pools.refused.empty()) throw Error(ABN_ERR_INVALID_ARG, pools.refused);
    if (pools.skipped) std::printf("Skipped %zu regions without a name in the 4th field\n", pools.skipped);
    if (pools.names.empty()) throw Error(ABN_ERR_INVALID_ARG, "No region of " + tiles.regions + " has a name to pool by");
  }
  // --region-states with --pool: every named row stays a tile of its own, the names are the groups — no sites are pooled
  const bool pooled = tiles.pool && !tiles.region.wanted;
  if (tiles.pool && !pooled) list = pools.rows;
  const char* unit = pooled ? "pool" : "tile";
  Owned<abn_tiles, abn_tiles_destroy> th;
  dev.check(abn_tiles_create(dev.get(), args.posterior_max_filter, (int32_t)args.align, (int32_t)nn,
                             resident::pointers(sites).data(), th.out()),
            "abn_tiles_create");
  for (const std::string& line : resident::align_report(args.align, names, resident::align_counts(th.get(), sites)))
    std::fputs(line.c_str(), stdout);
  if (tiles.fixed())
    dev.check(abn_tiles_set_fixed(th.get(), tiles.size, tiles.step), "abn_tiles_set_fixed");
  else if (pooled)
    dev.check(abn_tiles_set_pools(th.get(), (int64_t)pools.rows.size(), pools.rows.chromosome.data(), pools.rows.start.data(),
                                  pools.rows.end.data(), pools.pool.data(), (int64_t)pools.names.size()),
              "abn_tiles_set_pools");
  else
    dev.check(abn_tiles_set_intervals(th.get(), (int64_t)list.size(), list.chromosome.data(), list.start.data(), list.end.data()),
              "abn_tiles_set_intervals");
  int64_t n_tiles = 0;
  abn_tiles_info(th.get(), nullptr, nullptr, nullptr, nullptr, &n_tiles);
  const size_t T = (size_t)n_tiles;
  if (T == 0) throw Error(ABN_ERR_INVALID_ARG, "no tile: the methylomes hold no site");
  std::vector<int64_t> segments(T, 0);  // --pool: every pool's merged segments
  if (pooled) {
    int64_t S = 0;
    dev.check(abn_tiles_pool_segments(th.get(), &S, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "abn_tiles_pool_segments");
    std::vector<int32_t> of((size_t)S);
    dev.check(abn_tiles_pool_segments(th.get(), nullptr, of.data(), nullptr, nullptr, nullptr, nullptr, nullptr), "abn_tiles_pool_segments");
    for (int32_t p : of) ++segments[(size_t)p];
  } else {
    list.chromosome.resize(T), list.start.resize(T), list.end.resize(T);
    dev.check(abn_tiles_intervals(th.get(), list.chromosome.data(), list.start.data(), list.end.data()), "abn_tiles_intervals");
  }
  if (tiles.region.wanted) {  // of the tiles' own results only their sites are read: no per-tile fold or scan table here
    std::vector<int64_t> sites(T);
    dev.check(abn_tiles_stats(th.get(), sites.data(), nullptr, nullptr), "abn_tiles_stats");
    return regions_of_tiles(args, tiles, loaded, th.get(), list, sites, tiles.pool ? pools.pool.data() : nullptr,
                            tiles.pool ? pools.names : std::vector<std::string>{"regions"});
  }
  std::vector<int64_t> count(T), kept(nn * T);
  std::vector<double> sum(nn * T), dv(std::max<size_t>(T * npairs, 1), 0.0);
  std::vector<uint64_t> both(std::max<size_t>(T * npairs, 1), 0);
  dev.check(abn_tiles_stats(th.get(), count.data(), sum.data(), kept.data()), "abn_tiles_stats");
  dev.check(abn_tiles_pairwise(th.get(), nullptr, both.data(), dv.data()), "abn_tiles_pairwise");

  transitions::Table table;
  if (transitions::request().wanted) {
    for (const auto& node : graph.nodes) {
      table.names.push_back(node.name);
      table.generations.push_back(node.generation);
    }
    table.counts.assign(T * npairs * 9, 0);
    if (npairs > 0) dev.check(abn_tiles_transitions(th.get(), table.counts.data()), "abn_tiles_transitions");
  }

  const std::vector<detail::PairTimes> times = detail::convert_times(graph);
  std::vector<Win> wins;
  for (size_t t = 0; t < T; ++t) {
    const std::string region = pooled ? pools.names[t] : tile_region(list.chromosome[t], list.start[t], list.end[t]);
    try {
      if (count[t] == 0) throw Error(ABN_ERR_INVALID_ARG, std::string("no site lies in this ") + unit);
      for (size_t a = 0; a < nn; ++a)
        if (kept[a * T + t] == 0)
          throw Error(ABN_ERR_INVALID_ARG, names[a] + " has no site above the posterior filter in this " + unit);
      for (size_t a = 0, p = 0; a < nn; ++a)
        for (size_t b = a + 1; b < nn; ++b, ++p)
          if (both[t * npairs + p] == 0)
            throw Error(ABN_ERR_INVALID_ARG, names[a] + " and " + names[b] + " share no site above the posterior filter in this " + unit);
      wins.push_back(window_from_handle(region, t, times, sample_of, nn, T, t, sum, kept, &dv[t * npairs]));
    } catch (const std::exception& e) {
      std::printf("Error: Error while building pedigree: %s %zu (%s): %s\n", unit, t, region.c_str(), e.what());
    }
  }
  TilesOutput res;
  res.transitions = std::move(table);
  res.out = fit_windows(args, std::move(wins), std::vector<int>());
  if (tiles.block_replicates > 0)  // the blocks drawn with replacement: a pool's segments, or the genome's tiles in one group
    res.block = block_bootstrap(th.get(), pooled ? pools.names : std::vector<std::string>{"genome"}, times, sample_of, nn,
                                tiles.block_replicates, tiles.block_starts);
  std::vector<char> fitted(T, 0);
  res.out.results_txt = results_header();
  for (const WindowResult& r : res.out.results) {
    fitted[r.window_index] = 1;
    res.out.results_txt += results_line(args.name, r.window_index, (long long)count[r.window_index], r);
  }
  if (pooled) {
    res.pools_txt = "pool;name;intervals;segments;cg_count;fitted\n";
    for (size_t t = 0; t < T; ++t)
      res.pools_txt += std::to_string(t) + ";" + pools.names[t] + ";" + std::to_string(pools.intervals[t]) + ";" +
                       std::to_string(segments[t]) + ";" + std::to_string(count[t]) + ";" + (fitted[t] ? "1" : "0") + "\n";
    return res;
  }
  res.tiles_txt = "tile;chromosome;start;end;cg_count;fitted\n";
  for (size_t t = 0; t < T; ++t)
    res.tiles_txt += std::to_string(t) + ";" + chromosome_name(list.chromosome[t]) + ";" + std::to_string(list.start[t]) + ";" +
                     std::to_string(list.end[t]) + ";" + std::to_string(count[t]) + ";" + (fitted[t] ? "1" : "0") + "\n";
  return res;
}

// contexts: ONE methylation context (1 CG, the reference's; 2 CHG; 4 CHH) — the run on that context's sites
inline TilesOutput alphabeta_multiple_tiles(const WindowArgs& args, const TileArgs& tiles, unsigned contexts = 1u) {
  const TileSamples loaded = load_tile_samples(args, contexts);
  return tiles_of_samples(args, tiles, loaded, loaded.samples.sites);
}

// ... SEVERAL contexts: every methylome is read and parsed once and split on the device (abn_sites_split); each context is
// then built and fitted as the run under that context alone is — its own tiles, every tile's random stream at its index
// among that context's tiles — so each result is that run's, bit for bit.  done(c, result) as each context finishes.
template <class Done>
inline void alphabeta_multiple_tiles_contexts(const WindowArgs& args, const TileArgs& tiles, unsigned contexts, Done done) {
  const TileSamples loaded = load_tile_samples(args, contexts);
  const auto by_context = loaded.samples.split();
  for (size_t c = 0; c < 3; ++c)
    if ((contexts >> c) & 1u) done(c, tiles_of_samples(args, tiles, loaded, by_context[c]));
}

}  // namespace metaprofile
}  // namespace alphabeta
