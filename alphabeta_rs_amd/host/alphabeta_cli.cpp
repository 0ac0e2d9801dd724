// `alphabeta` command-line tool: same flags, console output and output files as the reference binary
// (src/cli/alphabeta.rs:8-38, src/arguments.rs:93-152), running the ABneutral path on an MI355X through
// libabneutral_hip.so.  Extra flags (not in the reference): --seed, --device(s), --lanes, --strict-order, --stream-sweep, --parse, --sites, --simulate (--sim-*), and
// --pedigree FILE --p0uu X to start from an existing pedigree file instead of nodelist/edgelist.
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <iostream>

#include "alphabeta.hpp"
#include "simulate.hpp"

namespace fs = std::filesystem;
using namespace alphabeta;

static void usage() {
  std::puts(
      "Usage: alphabeta [OPTIONS]\n\n"
      "Options:\n"
      "  -i, --iterations <ITERATIONS>  Number of iterations to run for Nelder-Mead optimization, even 100 is enough [default: 1000]\n"
      "  -e, --edges <EDGES>            Relative or absolute path to an edgelist, see /data for an example [default: ./edgelist.txt]\n"
      "  -n, --nodes <NODES>            Relative or absolute path to a nodelist, see /data for an example [default: ./nodelist.txt]\n"
      "  -p, --posterior-max-filter <P> Minimum posterior probability for a singe basepair read to be included in the estimation [default: 0.99]\n"
      "  -o, --output <OUTPUT>          Relative or absolute path to an output directory, must exist, EXISTING FILES WILL BE OVERWRITTEN [default: .]\n"
      "      --seed <SEED>              Philox seed of start simplices, jitter and bootstrap indices [default: 20260101]\n"
      "      --device <N>               HIP device ordinal [default: 0]\n"
      "      --devices <A,B,..>         several HIP devices: the bootstraps are sharded over them, tables gathered with RCCL\n"
      "      --lanes <G>                lanes of a wavefront per Nelder-Mead chain: 0 (auto), 8, 16, 32, 64\n"
      "      --strict-order             sum every cost's residuals serially in row order, exactly as the reference does\n"
      "                                 (src/structs.rs:206-213): bit-equal to a reference-order CPU run, ~1.5x the time\n"
      "      --stream-sweep             pedigrees too large for the LDS: read a fit's rows once per Nelder-Mead iteration\n"
      "                                 instead of once per cost evaluation; the same output files\n"
      "      --pedigree <FILE>          use this pedigree file (src/pedigree.rs:62-79 format) instead of building one\n"
      "      --p0uu <X>                 proportion of unmethylated sites at G0 (required with --pedigree)\n"
      "      --parse <host|device>      where the methylome files are parsed; the same output files [default: device]\n"
      "      --sites <host|device>      where the parsed sites wait for the pedigree build: device packs the codes and folds\n"
      "                                 the methylation levels there (needs --parse device); the same output files\n"
      "                                 [default: host]\n"
      "      --align <none|position|union>\n"
      "                                 position: compare the samples on the sites they all share, by chromosome, start,\n"
      "                                 end and strand; D and p0uu then describe the shared sites.  union: compare every\n"
      "                                 pair on the sites both samples hold; p0uu stays each file's own.  Both need\n"
      "                                 --sites device\n"
      "                                 [default: none]\n"
      "      --contexts <LIST>          the methylation contexts to fit, a comma-separated subset of CG,CHG,CHH (needs\n"
      "                                 --sites device).  One: the run on that context's sites.  Several: every methylome\n"
      "                                 is parsed once and each context is a run of its own, its files in <OUTPUT>/<CTX>/\n"
      "                                 [default: CG]\n"
      "      --sort                     sort every methylome by chromosome, start, end and strand on the device behind its\n"
      "                                 parse, so files in any line order are compared and aligned; a file that was out of\n"
      "                                 order is named in one line; the same output files as for the files sorted\n"
      "                                 beforehand (needs --sites device) [default: off]\n"
      "      --dedup <POLICY>           collapse the records of a methylome that repeat one (chromosome, start, end, strand)\n"
      "                                 on the device, behind the sort that --dedup implies: first or last keeps that record\n"
      "                                 of the file, best the one with the highest posteriormax (ties: the earlier), drop\n"
      "                                 none of a site called more than once; a file that held repeats is named in one\n"
      "                                 line (needs --sites device) [default: off; repeats are refused by --align position\n"
      "                                 and union]\n"
      "      --transitions              also write <OUTPUT>/transitions.txt: per pair of sampled nodes the sites both keep,\n"
      "                                 by status in the first and in the second sample (UU UI UM IU II IM MU MI MM)\n"
      "      --simulate <ALPHA,BETA>    fit methylomes simulated on the device under the ABneutral model at these rates: the\n"
      "                                 nodelist and the edgelist give the tree (one root, every other node one incoming\n"
      "                                 edge), the nodes with meth = Y are sampled, no methylome file is opened; needs\n"
      "                                 --sim-sites; --seed seeds the draws too [default: off]\n"
      "      --sim-sites <L>            sites of every simulated methylome\n"
      "      --sim-p0uu <P>             share of unmethylated sites in the founder's generation-0 ancestor [default: 0.75]\n"
      "      --sim-weight <W>           share of the founder's methylated sites that are epiheterozygous [default: 0.5]\n"
      "      --sim-replicates <R>       a replicate study: R independent pedigrees of --sim-sites sites from one simulation, all\n"
      "                                 fitted at once; the usual files are replicate 0's, simulation.txt has the mean, sd and\n"
      "                                 2.5 / 97.5 percentiles of the recovered rates, simulation_raw.npy every replicate's row\n"
      "      --sim-starts <S>           start simplices of every replicate's fit [default: 10]\n"
      "      --sim-miscall <E>          probability that a call differs from the true state, split evenly over the two other\n"
      "                                 states [default: 0]\n"
      "      --sim-dropout <F>          probability that a call is filtered, whatever the state [default: 0]\n"
      "  -h, --help                    Print help\n"
      "  -V, --version                  Print version");
}

int main(int argc, char** argv) {
  Args args;
  args.device_parse = true;  // measured: docs/experiments.md, "Device parsing"
  bool edges_given = false, nodes_given = false, contexts_given = false;
  std::string ped_file;
  double p0uu_given = -1.0;
  uint64_t seed = 20260101ull;
  simulate::Request sim;
  bool sites_given = false, parse_given = false, align_given = false, sim_option_given = false;
  bool study_option_given = false, replicates_given = false;
  int device = 0, lanes = 0;
  bool strict_order = false, stream_sweep = false;
  std::string devices_arg;
  auto need = [&](int& i) -> const char* {
    if (i + 1 >= argc) {
      std::fprintf(stderr, "error: a value is required for '%s' but none was supplied\n", argv[i]);
      std::exit(2);
    }
    return argv[++i];
  };
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i], v;
    auto eq = a.find('=');
    bool has_eq = a.rfind("--", 0) == 0 && eq != std::string::npos;
    if (has_eq) {
      v = a.substr(eq + 1);
      a = a.substr(0, eq);
    }
    auto val = [&]() -> std::string { return has_eq ? v : std::string(need(i)); };
    if (a == "-i" || a == "--iterations") args.iterations = (size_t)std::strtoull(val().c_str(), nullptr, 10);
    else if (a == "-e" || a == "--edges") { args.edges = val(); edges_given = true; }
    else if (a == "-n" || a == "--nodes") { args.nodes = val(); nodes_given = true; }
    else if (a == "-p" || a == "--posterior-max-filter") args.posterior_max_filter = std::strtod(val().c_str(), nullptr);
    else if (a == "-o" || a == "--output") args.output = val();
    else if (a == "--seed") seed = std::strtoull(val().c_str(), nullptr, 10);
    else if (a == "--device") device = std::atoi(val().c_str());
    else if (a == "--devices") devices_arg = val();
    else if (a == "--lanes") lanes = std::atoi(val().c_str());
    else if (a == "--strict-order") strict_order = true;
    else if (a == "--stream-sweep") stream_sweep = true;
    else if (a == "--pedigree") ped_file = val();
    else if (a == "--p0uu") p0uu_given = std::strtod(val().c_str(), nullptr);
    else if (a == "--simulate") {
      if (!simulate::parse_rates(val(), sim.alpha, sim.beta)) {
        std::fprintf(stderr, "error: %s\n", simulate::kSimulateExpects);
        return 2;
      }
      sim.wanted = true;
    }
    else if (a == "--sim-sites") { sim.sites = std::strtoll(val().c_str(), nullptr, 10); sim_option_given = true; }
    else if (a == "--sim-p0uu") { sim.p_uu0 = std::strtod(val().c_str(), nullptr); sim_option_given = true; }
    else if (a == "--sim-weight") { sim.weight = std::strtod(val().c_str(), nullptr); sim_option_given = true; }
    else if (a == "--sim-replicates") { sim.replicates = std::strtoll(val().c_str(), nullptr, 10); study_option_given = replicates_given = true; }
    else if (a == "--sim-starts") { sim.starts = std::atoi(val().c_str()); study_option_given = true; }
    else if (a == "--sim-miscall") { sim.miscall = std::strtod(val().c_str(), nullptr); study_option_given = true; }
    else if (a == "--sim-dropout") { sim.dropout = std::strtod(val().c_str(), nullptr); study_option_given = true; }
    else if (a == "--parse") {
      parse_given = true;
      const std::string where = val();
      if (where != "host" && where != "device") {
        std::fprintf(stderr, "error: --parse expects host or device\n");
        return 2;
      }
      args.device_parse = where == "device";
    }
    else if (a == "--sites") {
      sites_given = true;
      const std::string where = val();
      if (where != "host" && where != "device") {
        std::fprintf(stderr, "error: --sites expects host or device\n");
        return 2;
      }
      args.device_sites = where == "device";
    }
    else if (a == "--align") {
      align_given = true;
      const std::string how = val();
      if (!alphabeta::parse_align(how, args.align)) {
        std::fprintf(stderr, "error: %s\n", alphabeta::kAlignExpects);
        return 2;
      }
    }
    else if (a == "--contexts") {
      if (!resident::parse_contexts(val(), args.contexts)) {
        std::fprintf(stderr, "error: %s\n", resident::kContextsExpects);
        return 2;
      }
      contexts_given = true;
    }
    else if (a == "--sort") args.sort = true;
    else if (a == "--dedup") {
      if ((args.dedup = resident::parse_dedup(val())) < 0) {
        std::fprintf(stderr, "error: %s\n", resident::kDedupExpects);
        return 2;
      }
    }
    else if (a == "--transitions") transitions::request().wanted = true;
    else if (a == "-h" || a == "--help") { usage(); return 0; }
    else if (a == "-V" || a == "--version") { std::puts("alphabeta 0.2.1 (MI355X ABneutral path)"); return 0; }
    else {
      std::fprintf(stderr, "error: unexpected argument '%s' found\n\nFor more information, try '--help'.\n", argv[i]);
      return 2;
    }
  }
  if (sim_option_given && !sim.wanted) {
    std::fprintf(stderr, "error: --sim-sites, --sim-p0uu and --sim-weight belong to --simulate\n");
    return 2;
  }
  if (study_option_given && !sim.wanted) {
    std::fprintf(stderr, "error: --sim-replicates, --sim-starts, --sim-miscall and --sim-dropout belong to --simulate\n");
    return 2;
  }
  if (study_option_given && !replicates_given) {
    std::fprintf(stderr, "error: --sim-starts, --sim-miscall and --sim-dropout belong to --sim-replicates\n");
    return 2;
  }
  if (sim.wanted) {  // the methylomes are simulated: nothing that reads, orders or aligns methylome files applies
    const std::pair<bool, const char*> excluded[] = {
        {sites_given, "--sites"}, {parse_given, "--parse"}, {contexts_given, "--contexts"}, {args.sort, "--sort"},
        {args.dedup >= 0, "--dedup"}, {align_given, "--align"}, {!ped_file.empty(), "--pedigree"}};
    for (const auto& x : excluded)
      if (x.first) {
        std::fprintf(stderr, "error: --simulate cannot be combined with %s: the methylomes are simulated\n", x.second);
        return 2;
      }
    if (transitions::request().wanted) {
      std::fprintf(stderr, "error: --simulate cannot be combined with --transitions\n");
      return 2;
    }
    if (sim.sites < 1) {
      std::fprintf(stderr, "error: --simulate needs --sim-sites, a positive number of sites\n");
      return 2;
    }
    if (replicates_given) {
      const std::string why = simulate::study_refusal(sim);
      if (!why.empty()) {
        std::fprintf(stderr, "error: %s\n", why.c_str());
        return 2;
      }
    }
  }
  if (contexts_given && !(args.device_sites && args.device_parse)) {
    std::fprintf(stderr, "error: --contexts needs --sites device and --parse device\n");
    return 2;
  }
  if (args.sort && !(args.device_sites && args.device_parse)) {
    std::fprintf(stderr, "error: --sort needs --sites device and --parse device\n");
    return 2;
  }
  if (args.sort && !ped_file.empty()) {
    std::fprintf(stderr, "error: --sort belongs to --nodes and --edges: a pedigree file holds no methylome\n");
    return 2;
  }
  if (args.dedup >= 0 && !(args.device_sites && args.device_parse)) {
    std::fprintf(stderr, "error: --dedup needs --sites device and --parse device\n");
    return 2;
  }
  if (args.dedup >= 0 && !ped_file.empty()) {
    std::fprintf(stderr, "error: --dedup belongs to --nodes and --edges: a pedigree file holds no methylome\n");
    return 2;
  }
  if (args.device_sites && !args.device_parse) {
    std::fprintf(stderr, "error: --sites device needs --parse device\n");
    return 2;
  }
  if (args.align != alphabeta::Align::None && !args.device_sites) {
    std::fprintf(stderr, "error: --align %s needs --sites device\n", alphabeta::align_name(args.align));
    return 2;
  }
  if (transitions::request().wanted && !ped_file.empty()) {
    std::fprintf(stderr, "error: --transitions belongs to --nodes and --edges\n");
    return 2;
  }
  if (args.device_sites && !ped_file.empty()) {
    std::fprintf(stderr, "error: --sites belongs to --nodes and --edges\n");
    return 2;
  }
  (void)edges_given;
  (void)nodes_given;
  // value parsers of src/arguments.rs:116-140
  if (ped_file.empty()) {
    for (const std::string* f : {&args.edges, &args.nodes}) {
      if (fs::exists(*f)) std::printf("Using default file: %s\n", f->c_str());
      else {
        std::fprintf(stderr, "error: Please provide a valid file path. By default, we fill try %s, which does not exist.\n", f->c_str());
        return 2;
      }
    }
  }
  if (fs::exists(args.output)) std::printf("Using default output directory: %s\n", fs::canonical(args.output).c_str());
  else {
    std::fprintf(stderr, "error: Please provide a valid output directory. By default, we fill try %s, which does not exist.\n", args.output.c_str());
    return 2;
  }
  if (args.iterations == 0) {
    std::fprintf(stderr, "error: --iterations must be positive\n");
    return 2;
  }
  try {
    if (!devices_arg.empty()) {
      device_list() = parse_device_list(devices_arg);
      device = device_list()[0];
    }
    Device& dev = default_device(device);
    if (device_list().empty()) device_list().push_back(device);
    dev.options.seed = seed;
    dev.options.lanes_per_chain = lanes;
    dev.options.strict_order = strict_order ? 1 : 0;
    dev.stream_sweep = stream_sweep;
    // src/cli/alphabeta.rs:19-35
    auto report = [](const RunResult& r, const fs::path& out) {
      std::printf("##########\nResults:\n\n%s\n%s\n", r.model.display().c_str(), r.analysis.display().c_str());
      std::printf("Estimated steady state %s\n", fmt_f64(steady_state(r.model.alpha, r.model.beta)).c_str());
      std::printf("Observed steady state methylation %s\n##########\n", fmt_f64(r.obs_steady_state).c_str());
      r.pedigree.to_file((out / "pedigree.txt").string());
      r.analysis.to_file((out / "analysis.txt").string());
      r.raw_analysis.write_npy((out / "raw.npy").string());
    };
    // --transitions: the k-th pedigree build's table
    auto report_transitions = [](size_t k, const fs::path& out) {
      if (transitions::request().wanted) transitions::write_txt((out / "transitions.txt").string(), transitions::request().tables.at(k));
    };
    if (!resident::one_context(args.contexts)) {  // every context a run of its own, its files in <output>/<CTX>/
      size_t k = 0;
      run_contexts(args, [&](size_t c, const RunResult& r) {
        const fs::path out = fs::path(args.output) / resident::kContextNames[c];
        fs::create_directories(out);
        std::printf("Context %s\n", resident::kContextNames[c]);
        report(r, out);
        report_transitions(k++, out);
      });
      return 0;
    }
    RunResult r;
    if (!ped_file.empty()) {
      if (!(p0uu_given > 0.0 && p0uu_given < 1.0)) {
        std::fprintf(stderr, "error: --pedigree needs --p0uu in (0,1)\n");
        return 2;
      }
      r = run_on_pedigree(Pedigree::from_file(ped_file), p0uu_given, args.iterations, args.output);
    } else if (sim.wanted && sim.replicates > 0) {
      std::printf("Simulating pedigree...\n");
      simulate::Study st = simulate::study(sim, args.nodes, args.edges, seed);
      r = run_on_pedigree(std::move(st.pedigree), st.p0uu, args.iterations, args.output);
      std::printf("Replicates with a finite fit: %zu of %lld\n", st.ok, sim.replicates);
      std::ofstream((fs::path(args.output) / "simulation.txt").string()) << st.txt;
      st.raw.write_npy((fs::path(args.output) / "simulation_raw.npy").string());
    } else if (sim.wanted) {
      std::printf("Simulating pedigree...\n");
      auto [pedigree, p0uu] = simulate::build(sim, args.nodes, args.edges, seed);
      r = run_on_pedigree(std::move(pedigree), p0uu, args.iterations, args.output);
    } else {
      r = run(args);
    }
    report(r, fs::path(args.output));
    report_transitions(0, fs::path(args.output));
  } catch (const Error& e) {
    std::printf("Error: %s\n", e.what());  // src/cli/alphabeta.rs:17 prints and exits 0; a status is more useful
    return 1;
  }
  return 0;
}
