// `metaprofile_alphabeta`: the reference's `metaprofile` binary (src/cli/metaprofile.rs:33-114).
// Without --methylome: the AlphaBeta stage on window directories that already exist
// (<output-dir>/{upstream,gene,downstream}/<window>/{nodelist,edgelist}.txt, as written by src/setup.rs:35-72).
// With --methylome DIR --genome FILE --nodes FILE --edges FILE: the `extract` stage too (src/extract.rs:17-155), from
// whole methylome files and a gene annotation, the sites placed into windows on the device and no file tree in between.
// With --methylome DIR --nodes FILE --edges FILE and --tiles SIZE [--tile-step STEP] or --regions FILE: the rates per
// genomic tile (tiles.hpp) — fixed bins along the genome or the rows of a BED-like list — from whole methylomes kept on the
// device; no annotation.  With --regions FILE --pool: one pedigree per name in the list's 4th field.  With --region-states
// LO,HI: every tile or row gets one state per sample and the pedigree is built from the regions' states (region_states.hpp).
// All windows are fitted by one batched plan on the MI355X.  Flags follow src/arguments.rs:6-62 where they apply.
#include <cstdlib>
#include <cstring>
#include <filesystem>

#include "tiles.hpp"

using namespace alphabeta;

int main(int argc, char** argv) {
  metaprofile::WindowArgs a;
  a.device_parse = true;  // measured: docs/experiments.md, "Device parsing"
  a.device_genes = true;  // measured: docs/experiments.md, "Gene choice on the device"
  uint32_t max_gene_length = 0;
  std::string dist_file;
  uint64_t seed = 20260101ull;
  int device = 0;
  std::string devices_arg;
  bool stream_sweep = false;
  metaprofile::TileArgs tiles;
  bool region_min_given = false;
  bool tiles_given = false, tile_step_given = false, block_starts_given = false, parse_host = false, sites_host = false, contexts_given = false;
  unsigned contexts = 1u;
  for (int i = 1; i < argc; ++i) {
    const std::string f = argv[i];
    auto val = [&]() -> std::string {
      if (i + 1 >= argc) {
        std::fprintf(stderr, "error: a value is required for '%s'\n", argv[i]);
        std::exit(2);
      }
      return argv[++i];
    };
    if (f == "-o" || f == "--output-dir") a.output_dir = val();
    else if (f == "--name") a.name = val();
    else if (f == "-s" || f == "--window-step") a.window_step = (uint32_t)std::strtoul(val().c_str(), nullptr, 10);
    else if (f == "-w" || f == "--window-size") a.window_size = (uint32_t)std::strtoul(val().c_str(), nullptr, 10);
    else if (f == "-c" || f == "--cutoff") a.cutoff = (uint32_t)std::strtoul(val().c_str(), nullptr, 10);
    else if (f == "-a" || f == "--absolute") a.absolute = true;
    else if (f == "--iterations") a.iterations = (size_t)std::strtoull(val().c_str(), nullptr, 10);
    else if (f == "--max-gene-length") max_gene_length = (uint32_t)std::strtoul(val().c_str(), nullptr, 10);
    else if (f == "--distribution") dist_file = val();
    else if (f == "--seed") seed = std::strtoull(val().c_str(), nullptr, 10);
    else if (f == "--device") device = std::atoi(val().c_str());
    else if (f == "--devices") devices_arg = val();
    else if (f == "-m" || f == "--methylome") a.methylome = val();
    else if (f == "-g" || f == "--genome") a.genome = val();
    else if (f == "--nodes") a.nodes = val();
    else if (f == "--edges") a.edges = val();
    else if (f == "--cutoff-gene-length") a.cutoff_gene_length = true;
    else if (f == "--stream-sweep") stream_sweep = true;
    else if (f == "-i" || f == "--invert") a.invert = true;
    else if (f == "--parse") {
      const std::string where = val();
      if (where != "host" && where != "device") {
        std::fprintf(stderr, "error: --parse expects host or device\n");
        return 2;
      }
      a.device_parse = where == "device";
      parse_host = !a.device_parse;
    }
    else if (f == "--genes") {
      const std::string where = val();
      if (where != "host" && where != "device") {
        std::fprintf(stderr, "error: --genes expects host or device\n");
        return 2;
      }
      a.device_genes = where == "device";
    }
    else if (f == "--sites") {
      const std::string where = val();
      if (where != "host" && where != "device") {
        std::fprintf(stderr, "error: --sites expects host or device\n");
        return 2;
      }
      a.device_sites = where == "device";
      sites_host = !a.device_sites;
    }
    else if (f == "--align") {
      const std::string how = val();
      if (!alphabeta::parse_align(how, a.align)) {
        std::fprintf(stderr, "error: %s\n", alphabeta::kAlignExpects);
        return 2;
      }
    }
    else if (f == "--tiles" || f == "--tile-step") {
      const std::string v = val();
      char* e = nullptr;
      const long long n = std::strtoll(v.c_str(), &e, 10);
      if (v.empty() || *e != 0 || n < (f == "--tiles" ? 1 : 0)) {
        std::fprintf(stderr, "error: %s expects a number of base pairs%s\n", f.c_str(), f == "--tiles" ? " above 0" : "");
        return 2;
      }
      (f == "--tiles" ? tiles.size : tiles.step) = n;
      (f == "--tiles" ? tiles_given : tile_step_given) = true;
    }
    else if (f == "--contexts") {
      if (!resident::parse_contexts(val(), contexts)) {
        std::fprintf(stderr, "error: %s\n", resident::kContextsExpects);
        return 2;
      }
      contexts_given = true;
    }
    else if (f == "--block-bootstrap" || f == "--block-starts") {
      const std::string v = val();
      char* e = nullptr;
      const long long n = std::strtoll(v.c_str(), &e, 10);
      const long long most = f == "--block-starts" ? 1000000 : (1ll << 20) - 2;
      if (v.empty() || *e != 0 || n < 1 || n > most) {
        std::fprintf(stderr, "error: %s expects a number from 1 to %lld\n", f.c_str(), most);
        return 2;
      }
      if (f == "--block-starts") tiles.block_starts = (int)n, block_starts_given = true;
      else tiles.block_replicates = n;
    }
    else if (f == "--sort") a.sort = true;
    else if (f == "--dedup") {
      if ((a.dedup = resident::parse_dedup(val())) < 0) {
        std::fprintf(stderr, "error: %s\n", resident::kDedupExpects);
        return 2;
      }
    }
    else if (f == "--regions") tiles.regions = val();
    else if (f == "--region-states") {
      if (!metaprofile::parse_region_states(val(), tiles.region)) {
        std::fprintf(stderr, "error: %s\n", metaprofile::kRegionStatesExpects);
        return 2;
      }
      tiles.region.wanted = true;
    }
    else if (f == "--region-min-sites") {
      if (!metaprofile::parse_region_min_sites(val(), tiles.region.min_sites)) {  // digits only, as LO,HI
        std::fprintf(stderr, "error: --region-min-sites expects a number of sites of at least 1\n");
        return 2;
      }
      region_min_given = true;
    }
    else if (f == "--pool") tiles.pool = true;
    else if (f == "--transitions") transitions::request().wanted = true;
    else if (f == "-h" || f == "--help") {
      std::puts("Usage: metaprofile_alphabeta -o <output-dir> [--name N] [-s step] [-w size] [-c cutoff] [-a]\n"
                "       [--iterations 100] [--max-gene-length L] [--distribution FILE] [--seed S] [--device D]\n"
                "       [--devices A,B,..]   windows sharded over several HIP devices, tables gathered with RCCL\n"
                "       [--methylome DIR --genome FILE --nodes FILE --edges FILE [--cutoff-gene-length]]\n"
                "                            extract the windows from whole methylomes on the device (no window directories)\n"
                "       [--parse host|device] where the methylome files are parsed; the same output files [default: device]\n"
                "       [--genes host|device] where every site's gene is chosen; the same output files [default: device]\n"
                "       [--sites host|device] where the parsed sites wait for the gene choice: device keeps them there from the\n"
                "                            text to the window matrix (needs --parse device --genes device); the same output\n"
                "                            files [default: host]\n"
                "       [--align none|position|union] position: place only the sites every sample shares, by chromosome,\n"
                "                            start, end and strand; the side files then describe the shared sites.  union: give\n"
                "                            every sample all the sites any sample holds, filtered placeholders where it lacks\n"
                "                            one; the side files then count union sites.  Either way no window is ragged (needs\n"
                "                            --sites device) [default: none]\n"
                "       --methylome DIR --nodes FILE --edges FILE (--tiles SIZE [--tile-step STEP] | --regions FILE)\n"
                "                            rates per genomic tile instead of gene-relative windows: fixed tiles of SIZE bp\n"
                "                            every STEP bp along every chromosome [STEP default: SIZE], or the regions of a\n"
                "                            BED-like FILE (chromosome, start, end; half-open on a site's start).  Needs no\n"
                "                            --genome; the methylomes are parsed and kept on the device; --align as above,\n"
                "                            none expects the same sites in every methylome.  Writes results.txt (window = the\n"
                "                            tile's index, region = chromosome:start-end), raw.npy and tiles.txt\n"
                "       [--pool]             with --regions: the rows that share a name (4th field) are one pool, one pedigree of\n"
                "                            every site inside any of them, each site once - one rate per annotation class.\n"
                "                            Pools are numbered by first appearance; rows without a name are skipped.  Writes\n"
                "                            results.txt (window = the pool's index, region = its name), raw.npy and pools.txt\n"
                "       [--contexts LIST]    with --tiles or --regions: the methylation contexts to fit, a comma-separated subset\n"
                "                            of CG,CHG,CHH [default: CG].  One: the run on that context's sites.  Several: every\n"
                "                            methylome is parsed once and each context is a run of its own, its files in\n"
                "                            <output-dir>/<CTX>/\n"
                "       [--sort]             with --tiles or --regions, or with --genome --sites device: sort every methylome by\n"
                "                            chromosome, start, end and strand on the device behind its parse, so files in any\n"
                "                            line order (sorted by strand first, contigs in pieces, chromosomes in another order)\n"
                "                            are tiled and aligned; a file that was out of order is named in one line; the same\n"
                "                            output files as for the files sorted beforehand [default: off]\n"
                "       [--dedup POLICY]     where --sort is accepted, and implying it: collapse the records of a methylome that\n"
                "                            repeat one (chromosome, start, end, strand) on the device.  first or last keeps that\n"
                "                            record of the file, best the one with the highest posteriormax (ties: the earlier),\n"
                "                            drop none of a site called more than once; a file that held repeats is named in one\n"
                "                            line [default: off; repeats are refused by --align position and union]\n"
                "       [--transitions]      with --tiles or --regions: also write transitions.npy (uint64, tiles x pairs x 9: per\n"
                "                            tile and pair of sampled nodes the sites both keep, by status in the first and in\n"
                "                            the second sample, UU UI UM IU II IM MU MI MM) and transition_pairs.txt (sample_a,\n"
                "                            sample_b, generation_a, generation_b per pair); rows as tiles.txt / pools.txt\n"
                "       [--block-bootstrap R [--block-starts S]]  with --regions FILE --pool (one group per pool) or --tiles SIZE\n"
                "                            whose tiles do not overlap (one group, `genome`): draw the blocks - a pool's merged\n"
                "                            segments, the genome's tiles - with replacement R times per group, refit every draw\n"
                "                            from S starts [default 10], and write block_bootstrap.txt (per group alpha and beta\n"
                "                            of the observed data, sd and percentile CI of the draws) and block_raw.npy (R x 7 x\n"
                "                            groups); the other files stay as they are; one device\n"
                "       [--region-states LO,HI [--region-min-sites K]]  with --tiles or --regions: region-level analysis.  Every\n"
                "                            tile or row gets ONE state per sample, called on the device from the sample's sites\n"
                "                            inside it - their mean level (U 0, I 1/2, M 1) below LO calls U, above HI calls M,\n"
                "                            else I; fewer than K kept sites [default 1]: filtered - and ONE pedigree is built\n"
                "                            from all regions' states; with --pool one per name in the 4th field, the rows staying\n"
                "                            one region each (they may overlap).  LO and HI: decimals in [0, 1], at most six\n"
                "                            fraction digits, read exactly.  Writes results.txt (window = the group, cg_count = its\n"
                "                            regions), raw.npy, regions.txt, region_states.npy (uint8, samples x regions) and with\n"
                "                            --pool groups.txt; not with --block-bootstrap\n"
                "       [--stream-sweep]     pedigrees too large for the LDS: read a fit's rows once per Nelder-Mead iteration\n"
                "                            instead of once per cost evaluation; the same output files");
      return 0;
    } else {
      std::fprintf(stderr, "error: unexpected argument '%s' found\n", argv[i]);
      return 2;
    }
  }
  if (!std::filesystem::exists(a.output_dir)) {
    std::fprintf(stderr, "error: output directory %s does not exist\n", a.output_dir.c_str());
    return 2;
  }
  if (tiles.pool && tiles.regions.empty()) {
    std::fprintf(stderr, "error: --pool belongs to --regions\n");
    return 2;
  }
  const bool tile_mode = tiles_given || tile_step_given || !tiles.regions.empty();
  if (contexts_given) {
    const char* refused = nullptr;
    if (parse_host || sites_host) refused = "--contexts keeps the sites on the device: --parse host and --sites host do not apply";
    else if (a.methylome.empty()) refused = "--contexts belongs to --methylome with --tiles or --regions, not to window directories";
    else if (!tile_mode) refused = "--contexts belongs to --tiles and --regions, not to the gene windows of --genome";
    if (refused) {
      std::fprintf(stderr, "error: %s\n", refused);
      return 2;
    }
  }
  if (a.sort) {
    const char* refused = nullptr;
    if (parse_host || sites_host) refused = "--sort sorts the sites on the device: --parse host and --sites host do not apply";
    else if (a.methylome.empty()) refused = "--sort belongs to --methylome, not to window directories";
    else if (!tile_mode && !a.device_sites) refused = "--sort with the gene windows of --genome needs --sites device";
    if (refused) {
      std::fprintf(stderr, "error: %s\n", refused);
      return 2;
    }
  }
  if (a.dedup >= 0) {
    const char* refused = nullptr;
    if (parse_host || sites_host) refused = "--dedup collapses the sites on the device: --parse host and --sites host do not apply";
    else if (a.methylome.empty()) refused = "--dedup belongs to --methylome, not to window directories";
    else if (!tile_mode && !a.device_sites) refused = "--dedup with the gene windows of --genome needs --sites device";
    if (refused) {
      std::fprintf(stderr, "error: %s\n", refused);
      return 2;
    }
  }
  if (tiles.block_replicates > 0 || block_starts_given) {
    const char* refused = nullptr;
    if (tiles.block_replicates == 0) refused = "--block-starts belongs to --block-bootstrap";
    else if (!tile_mode) refused = "--block-bootstrap belongs to --regions FILE --pool and to --tiles SIZE";
    else if (!tiles.regions.empty() && !tiles.pool)
      refused = "--block-bootstrap with --regions needs --pool: the rows of a region list may overlap";
    else if (tiles_given && tiles.step != 0 && tiles.step < tiles.size)
      refused = "--block-bootstrap needs tiles that do not overlap: a --tile-step of at least the tile size";
    else if (devices_arg.find(',') != std::string::npos) refused = "--block-bootstrap runs on one device: --devices names several";
    if (refused) {
      std::fprintf(stderr, "error: %s\n", refused);
      return 2;
    }
  }
  if (tiles.region.wanted || region_min_given) {
    const char* refused = nullptr;
    if (!tiles.region.wanted) refused = "--region-min-sites belongs to --region-states";
    else if (!tile_mode || !a.genome.empty()) refused = "--region-states belongs to --tiles and --regions";
    else if (tiles.block_replicates > 0) refused = "--region-states does not go with --block-bootstrap: block resampling of regions is not built";
    if (refused) {
      std::fprintf(stderr, "error: %s\n", refused);
      return 2;
    }
  }
  if (transitions::request().wanted && !tile_mode) {
    std::fprintf(stderr, "error: --transitions belongs to --tiles and --regions\n");
    return 2;
  }
  if (tile_mode) {
    const char* refused = nullptr;
    if (tiles_given && !tiles.regions.empty()) refused = "--tiles and --regions exclude each other";
    else if (!tiles_given && tiles.regions.empty()) refused = "--tile-step belongs to --tiles";
    else if (a.methylome.empty() || a.nodes.empty() || a.edges.empty()) refused = "--tiles and --regions need --methylome, --nodes and --edges";
    else if (!a.genome.empty() || a.absolute || a.cutoff_gene_length || a.invert)
      refused = "--genome, -a, --cutoff-gene-length and --invert do not apply to --tiles and --regions";
    else if (parse_host || sites_host) refused = "--tiles and --regions keep the sites on the device: --parse host and --sites host do not apply";
    if (refused) {
      std::fprintf(stderr, "error: %s\n", refused);
      return 2;
    }
    a.device_sites = true;
  }
  if (tiles.pool) {  // a name the output files cannot hold is a flag error, before anything runs
    std::string refused;
    try {
      refused = metaprofile::region_pools(metaprofile::read_regions(detail::read_file(tiles.regions, "regions"))).refused;
    } catch (const Error&) {  // an unreadable list: the run says so
    }
    if (!refused.empty()) {
      std::fprintf(stderr, "error: %s\n", refused.c_str());
      return 2;
    }
  }
  const bool in_memory = !a.methylome.empty();
  if (in_memory && a.invert) {
    std::fprintf(stderr, "error: --invert is not supported with --methylome\n");
    return 2;
  }
  if (in_memory && !tile_mode && (a.genome.empty() || a.nodes.empty() || a.edges.empty())) {
    std::fprintf(stderr, "error: --methylome needs --genome, --nodes and --edges\n");
    return 2;
  }
  if (!in_memory && (!a.genome.empty() || !a.nodes.empty() || !a.edges.empty() || a.cutoff_gene_length || a.invert)) {
    std::fprintf(stderr, "error: --genome, --nodes, --edges, --cutoff-gene-length and --invert belong to --methylome\n");
    return 2;
  }
  if (a.device_sites && !(a.device_parse && a.device_genes)) {
    std::fprintf(stderr, "error: --sites device needs --parse device and --genes device\n");
    return 2;
  }
  if (a.align != alphabeta::Align::None && !a.device_sites) {
    std::fprintf(stderr, "error: --align %s needs --sites device\n", alphabeta::align_name(a.align));
    return 2;
  }
  if (a.device_sites && !in_memory) {
    std::fprintf(stderr, "error: --sites belongs to --methylome\n");
    return 2;
  }
  std::printf("Starting run %s\n", a.name.c_str());
  try {
    if (!devices_arg.empty()) {
      device_list() = parse_device_list(devices_arg);
      device = device_list()[0];
    }
    Device& dev = default_device(device);
    if (device_list().empty()) device_list().push_back(device);
    dev.options.seed = seed;
    dev.stream_sweep = stream_sweep;
    if (tile_mode) {
      auto write = [&](const metaprofile::TilesOutput& res, const std::filesystem::path& dir) {
        std::printf("%s\n", res.out.results_txt.c_str());
        std::ofstream(dir / "results.txt") << res.out.results_txt;
        if (tiles.region.wanted) {
          std::ofstream(dir / "regions.txt") << res.regions_txt;
          if (tiles.pool) std::ofstream(dir / "groups.txt") << res.groups_txt;
          metaprofile::write_u8_npy(res.region_states, res.region_rows, res.region_columns, (dir / "region_states.npy").string());
        } else if (tiles.pool) std::ofstream(dir / "pools.txt") << res.pools_txt;
        else std::ofstream(dir / "tiles.txt") << res.tiles_txt;
        metaprofile::write_raw_npy(res.out, (dir / "raw.npy").string());
        if (transitions::request().wanted) transitions::write_npy(dir.string(), res.transitions);
        if (tiles.block_replicates > 0) {
          std::ofstream(dir / "block_bootstrap.txt") << res.block.txt;
          metaprofile::write_block_raw_npy(res.block, (dir / "block_raw.npy").string());
        }
      };
      if (resident::one_context(contexts)) {
        write(metaprofile::alphabeta_multiple_tiles(a, tiles, contexts), a.output_dir);
        return 0;
      }
      // every context a run of its own on one parse of every methylome, its files in <output-dir>/<CTX>/
      metaprofile::alphabeta_multiple_tiles_contexts(a, tiles, contexts, [&](size_t c, const metaprofile::TilesOutput& res) {
        const std::filesystem::path dir = std::filesystem::path(a.output_dir) / resident::kContextNames[c];
        std::filesystem::create_directories(dir);
        std::printf("Context %s\n", resident::kContextNames[c]);
        write(res, dir);
      });
      return 0;
    }
    if (in_memory) {
      const auto ex = metaprofile::extract_in_memory(a);
      const auto out = metaprofile::alphabeta_multiple_in_memory(a, ex);
      std::printf("%s\n", out.results_txt.c_str());
      std::ofstream(std::filesystem::path(a.output_dir) / "results.txt") << out.results_txt;
      metaprofile::write_raw_npy(out, (std::filesystem::path(a.output_dir) / "raw.npy").string());
      return 0;
    }
    std::vector<int> distribution;
    if (!dist_file.empty()) {
      std::ifstream f(dist_file);
      int v;
      while (f >> v) distribution.push_back(v);
    } else {
      distribution.assign(100000, 0);  // cg_count column is filled by the extraction step, which is not part of this tool
    }
    const auto out = metaprofile::alphabeta_multiple(a, max_gene_length, distribution);
    std::printf("%s\n", out.results_txt.c_str());
    std::ofstream(std::filesystem::path(a.output_dir) / "results.txt") << out.results_txt;
    metaprofile::write_raw_npy(out, (std::filesystem::path(a.output_dir) / "raw.npy").string());
  } catch (const Error& e) {
    std::printf("Error: %s\n", e.what());
    return 1;
  }
  return 0;
}
