// stats -- maximum-likelihood statistics with the reference tool's options (aku/stats.cc:321-356) on
// the engine: features per utterance on the device, .phn segmentations on the host, the accumulation
// for many utterances per launch (aasr_run_stats_recipe), dumps as HmmSet::dump_statistics writes them.
//
//   stats (-b BASE | -g GK -m MC -p PH) -c CFG -r RECIPE -o OUT --ml [--full-stats] [-t] [-O] [-S SPKC [-U]] [-n]
//         [-B n -I k] [-i level] [--networks [-F fw] [-W bw] [-A scale] [-M bw|vit] [-a]]
//
// --full-stats (an extension of this tool, like --device) collects the full second moments sum gamma x x^T and writes
// mode-3 dumps, what estimate --mllt reads; pools of more than 127 dimensions are refused with it.
// --networks is the reference's -H under a spelling of its own: Baum-Welch (or with -M vit Viterbi) over the recipe's
// hmmnet= networks on the device, with -F / -W / -A honoured; -M mpv, --full-stats and -O are refused with it, and a
// recipe line without hmmnet= is the reference's error.  Without it -F / -W / -A / -M are read and ignored, as before.
// With --networks -M vit, -a writes every utterance's best path as a state-numbered alignment into the recipe line's
// alignment= file (what dur_est reads); -a under -M bw, with -O or without --networks is refused.
// Built: --ml over .phn files or networks.  -H itself (use --networks), --mmi / --mpe / --grad, --mllt, -P, --savelat
// and --nseggk / --nsegmc are refused before the device is opened, and so are full-covariance or
// subspace pools and speaker files with model transforms.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "tool_common.hh"

int main(int argc, char *argv[]) {
  aku::conf::Config config;
  config("usage: stats [OPTION...] --ml [--full-stats | --networks]\n")
    ('h', "help", "", "", "display help")
    ('b', "base=BASENAME", "arg", "", "base filename for model files")
    ('g', "gk=FILE", "arg", "", "Mixture base distributions")
    ('m', "mc=FILE", "arg", "", "Mixture coefficients for the states")
    ('p', "ph=FILE", "arg", "", "HMM definitions")
    ('\0', "nsegmc=FILE", "arg", "", "mc-file for segmentating the numerator")
    ('\0', "nseggk=FILE", "arg", "", "gk-file for segmentating the numerator")
    ('c', "config=FILE", "arg must", "", "feature configuration")
    ('r', "recipe=FILE", "arg must", "", "recipe file")
    ('O', "ophn", "", "", "use output phns for training")
    ('H', "hmmnet", "", "", "use HMM networks for training")
    ('o', "out=BASENAME", "arg must", "", "base filename for output statistics")
    ('t', "transitions", "", "", "collect also state transition statistics")
    ('F', "fw-beam=FLOAT", "arg", "0", "Forward beam (for HMM networks)")
    ('W', "bw-beam=FLOAT", "arg", "0", "Backward beam (for HMM networks)")
    ('A', "ac-scale=FLOAT", "arg", "1", "Acoustic scaling (for HMM networks)")
    ('\0', "num-mult=FLOAT", "arg", "1", "Loglikelihood multiplier for the numerator")
    ('M', "segmode=MODE", "arg", "bw", "Segmentation mode: bw/vit/mpv")
    ('\0', "numseg=MODE", "arg", "", "Numerator segmentation mode")
    ('\0', "ml", "", "", "Collect statistics for ML")
    ('\0', "mmi", "", "", "Collect statistics for MMI")
    ('\0', "mpe", "", "", "Collect statistics for MPE/MWE/MPFE")
    ('\0', "grad", "", "", "Prepare gradient based statistics (with --mpe)")
    ('\0', "mllt", "", "", "maximum likelihood linear transformation (for --ml)")
    ('\0', "errmode=MODE", "arg", "", "For --mpe. Modes: mwe/mpe/mpfe/mpfe-cps/mpfe-pdf/snfe")
    ('\0', "nosil=SIL", "arg", "", "Ignore silence arcs (labeled SIL) in MPE scoring")
    ('S', "speakers=FILE", "arg", "", "speaker configuration file")
    ('U', "uttadap", "", "", "Enable utterance adaptation")
    ('n', "no-train", "", "", "Only collect summary statistics")
    ('P', "precomplat", "", "", "Use precomputed segmented lattices (with rescoring)")
    ('\0', "savelat", "", "", "Don't train but only save segmented lattices")
    ('a', "alignment", "", "", "save output alignments (only with ML training)")
    ('B', "batch=INT", "arg", "0", "number of batch processes with the same recipe")
    ('I', "bindex=INT", "arg", "0", "batch process index")
    ('i', "info=INT", "arg", "0", "info level")
    ('\0', "device=INT", "arg", "-1", "GPU ordinal (default: the first visible device)")
    ('\0', "full-stats", "", "", "collect full second moments (mode-3 dumps, what estimate --mllt reads)")
    ('\0', "networks", "", "", "Baum-Welch over the recipe's hmmnet= networks; the reference's -H");
  config.default_parse(argc, argv);

  // what this build does not do, refused before anything is read
  const char *refused[][2] = {{"hmmnet", "-H (HMM network Baum-Welch)"},
                              {"mmi", "--mmi (discriminative statistics)"},
                              {"mpe", "--mpe (discriminative statistics)"},
                              {"grad", "--grad (discriminative statistics)"},
                              {"mllt", "--mllt"},
                              {"precomplat", "-P (precomputed lattices)"},
                              {"savelat", "--savelat"},
                              {"nseggk", "--nseggk (numerator segmentation model)"},
                              {"nsegmc", "--nsegmc (numerator segmentation model)"}};
  for (const auto &r : refused)
    if (config[r[0]].specified)
      die(std::string("stats: ") + r[1] + " is not supported; only --ml over .phn files is" +
          (std::string(r[0]) == "hmmnet" ? ", and over HMM networks with --networks" : ""));
  const bool networks = config["networks"].specified, alignment = config["alignment"].specified;
  const std::string segmode = config["segmode"].get_str();
  // -a: the best path's alignments, over networks only (aku/stats.cc:513-524)
  if (alignment && config["ophn"].specified) die("Can not read and write to output PHNs");
  if (alignment && !networks)
    die("stats: -a (alignment output) is not supported; only --ml over .phn files is, and -a over HMM networks with --networks -M vit");
  if (networks) {
    if (segmode == "mpv") die("stats: -M mpv (multipath Viterbi) is not supported with --networks; use -M bw or -M vit");
    if (segmode != "bw" && segmode != "vit") die("stats: -M " + segmode + ": invalid segmentation mode (bw, vit)");
    if (alignment && segmode != "vit")
      die("stats: -a (alignment output) needs -M vit with --networks: under Baum-Welch no single arc belongs to a frame");
    if (config["full-stats"].specified) die("stats: --full-stats is not supported with --networks");
    if (config["ophn"].specified) die("stats: -O (output phns) is not supported with --networks");  // (with -a: above)
  }

  std::string gk, mc, ph;
  resolve_model_files(config, &gk, &mc, &ph);
  if (config["batch"].specified ^ config["bindex"].specified) die("Must give both --batch and --bindex");
  if (!config["ml"].specified) die("At least one mode (--ml, --mmi, --mpe) must be given!");
  check_pool(gk, "stats");
  if (config["full-stats"].specified) {  // the full-statistics kernel's limit, known from the pool's header
    std::ifstream in(gk);
    int size = 0, dim = 0;
    in >> size >> dim;
    if (in && dim > 127)
      die("stats: --full-stats collects full second moments for at most 127 dimensions (" + gk + " has " +
          std::to_string(dim) + ")");
  }
  if (config["speakers"].specified) check_speakers(config["speakers"].get_str(), "stats");
  check_recipe_line_limits(config["recipe"].get_str(), config["batch"].get_int(), config["bindex"].get_int(), false,
                           "stats");
  if (networks)
    check_recipe_hmmnets(config["recipe"].get_str(), config["batch"].get_int(), config["bindex"].get_int(), false);

  const int device = config["device"].get_int();
  if (device >= 0 && aasr_set_device(device) != AASR_OK) die(aasr_last_error());

  const std::string cfg = config["config"].get_str();
  std::ifstream cin_(cfg);
  if (!cin_) die("could not open " + cfg);
  std::stringstream ss;
  ss << cin_.rdbuf();
  aasr_feat *feat = nullptr;
  aasr_gmm *gmm = nullptr;
  aasr_topo *topo = nullptr;
  if (aasr_feat_create(ss.str().c_str(), &feat) != AASR_OK) die(aasr_last_error());
  if (aasr_gmm_create_from_files(gk.c_str(), mc.c_str(), ph.c_str(), &gmm) != AASR_OK) die(aasr_last_error());
  if (aasr_topo_create_from_ph(ph.c_str(), &topo) != AASR_OK) die(aasr_last_error());

  aasr_stats_options opt;
  aasr_stats_default_options(&opt);
  opt.transitions = config["transitions"].specified;
  opt.ophn = config["ophn"].specified;
  opt.no_train = config["no-train"].specified;
  opt.uttadap = config["uttadap"].specified;
  opt.info = config["info"].get_int();
  opt.num_batches = config["batch"].get_int();
  opt.batch_index = config["bindex"].get_int();
  opt.full_stats = config["full-stats"].specified;
  aasr_stats_network_options nopt;
  aasr_stats_network_default_options(&nopt);
  nopt.viterbi = segmode == "vit";
  nopt.fw_beam = config["fw-beam"].get_float();
  nopt.bw_beam = config["bw-beam"].get_float();
  nopt.ac_scale = config["ac-scale"].get_float();
  nopt.ac_scale_given = config["ac-scale"].specified;
  nopt.alignment = alignment;
  const std::string out = config["out"].get_str();
  opt.out = out.c_str();
  aasr_spkc *spk = nullptr;
  if (config["speakers"].specified) {
    if (aasr_spkc_create(feat, gmm, &spk) != AASR_OK) die(aasr_last_error());
    if (aasr_spkc_read_file(spk, config["speakers"].get_str().c_str()) != AASR_OK) die(aasr_last_error());
  }
  opt.speakers = spk;
  aasr_run_stats st;
  memset(&st, 0, sizeof st);
  const std::string recipe = config["recipe"].get_str();
  if ((networks ? aasr_run_stats_networks_recipe(feat, gmm, topo, recipe.c_str(), &opt, &nopt, &st)
                : aasr_run_stats_recipe(feat, gmm, topo, recipe.c_str(), &opt, &st)) != AASR_OK)
    die(aasr_last_error());
  aasr_spkc_destroy(spk);
  aasr_topo_destroy(topo);
  aasr_gmm_destroy(gmm);
  aasr_feat_destroy(feat);
  return 0;
}
