// lda -- LDA estimation with the reference tool's options (aku/lda.cc:51-72) on the engine: per-state frame
// counts from the .phn segmentations on the host, the features at the transform module's source on the device, the
// states' scatter sums on the FP64 matrix pipe (aasr_run_lda_recipe), one host solve, the feature configuration
// with the module's new matrix.
//
//   lda -p PH -c CFG -r RECIPE -M MODULE [-d DIM] [-w OUT.cfg] [-O] [-S SPKC] [-m MB] [--mingamma G] [--maxgamma G]
//       [--no-silence] [-i level]
//       [--networks (-b BASE | -g GK --mc MC -p PH) [-F fw] [-W bw] [-A scale] [--segmode bw|vit]]
//
// --networks is the reference's -H under a spelling of its own: the states' sums from the Baum-Welch posteriors (or with
// --segmode vit the best paths) of the recipe's hmmnet= networks, scored with the model -b (or -g, --mc and -p; -m is
// this tool's --maxmem) names on the output of the whole feature chain (aasr_run_lda_networks_recipe), one pass, the
// selection made on the summed gamma.  -F, -W and -A are honoured with it; --segmode mpv and -O are refused with it, a
// recipe line without hmmnet= is the reference's error, and the module must have a matrix already.  The reference's
// own -H cannot run (it has no Gaussians to score with), so there is no binary to compare with.
//
// Refused before anything is read: -H, --mpv, --vit (HMM networks; use --networks), --segmode without --networks.
// Refused before the device is opened: recipe start-line / end-line, speaker files with model transforms, -d other
// than the module's dimension, a model without the _ or __ HMM, and with --networks non-diagonal pools.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "tool_common.hh"

int main(int argc, char *argv[]) {
  aku::conf::Config config;
  config("usage: lda [OPTION...]\n")
    ('h', "help", "", "", "display help")
    ('b', "base=BASENAME", "arg", "", "base filename for model files (with --networks)")
    ('g', "gk=FILE", "arg", "", "Mixture base distributions (with --networks)")
    ('\0', "mc=FILE", "arg", "", "Mixture coefficients for the states (with --networks)")
    ('p', "ph=FILE", "arg", "", "HMM definitions")
    ('c', "config=FILE", "arg must", "", "feature configuration")
    ('w', "write-config=FILE", "arg", "", "write feature configuration")
    ('r', "recipe=FILE", "arg must", "", "recipe file")
    ('O', "ophn", "", "", "use output phns for training")
    ('H', "hmmnet", "", "", "use HMM networks for training")
    ('d', "dim", "arg", "39", "dimensionality of the projected features (default 39)")
    ('M', "module=NAME", "arg", "", "linear transform module name")
    ('F', "fw-beam=FLOAT", "arg", "0", "Forward beam (for HMM networks)")
    ('W', "bw-beam=FLOAT", "arg", "0", "Backward beam (for HMM networks)")
    ('A', "ac-scale=FLOAT", "arg", "1", "Acoustic scaling (for HMM networks)")
    ('\0', "mpv", "", "", "Use Multipath Viterbi over HMM networks")
    ('\0', "vit", "", "", "Use Viterbi over HMM networks")
    ('S', "speakers=FILE", "arg", "", "speaker configuration file")
    ('m', "maxmem=INT", "arg", "3000", "maximum memory usage in MB (default 3000)")
    ('\0', "mingamma=FLOAT", "arg", "50", "minimum gamma value per state (default 50)")
    ('\0', "maxgamma=FLOAT", "arg", "1000000", "gamma values will be ceiled to maxgamma (default 1 000 000)")
    ('\0', "no-silence", "", "", "don't use silence states in estimation")
    ('i', "info=INT", "arg", "0", "info level")
    ('\0', "device=INT", "arg", "-1", "GPU ordinal (default: the first visible device)")
    ('\0', "networks", "", "", "segment with the recipe's hmmnet= networks; the reference's -H")
    ('\0', "segmode=MODE", "arg", "bw", "Segmentation mode with --networks: bw(default)/vit");
  config.default_parse(argc, argv);

  // what this build does not do, refused before anything is read
  const char *refused[][2] = {{"hmmnet", "-H (HMM network segmentation)"},
                              {"mpv", "--mpv (HMM network segmentation)"},
                              {"vit", "--vit (HMM network segmentation)"}};
  for (const auto &r : refused)
    if (config[r[0]].specified) die(std::string("lda: ") + r[1] + " is not supported; only .phn segmentations are");

  const bool networks = config["networks"].specified;
  const std::string segmode = config["segmode"].get_str();
  if (!networks && config["segmode"].specified)
    die("lda: --segmode is not supported without --networks; only .phn segmentations are");
  std::string gk, mc, ph;
  if (networks) {
    if (segmode == "mpv")
      die("lda: --segmode mpv (multipath Viterbi) is not supported with --networks; use --segmode bw or --segmode vit");
    if (segmode != "bw" && segmode != "vit") die("Invalid segmentation mode " + segmode);
    if (config["ophn"].specified) die("lda: -O (output phns) is not supported with --networks");
    resolve_model_files(config, &gk, &mc, &ph);
    check_pool(gk, "lda");
    check_recipe_hmmnets(config["recipe"].get_str(), 1, 1, true);
  } else {
    if (!config["ph"].specified) die("Must give --ph");
    ph = config["ph"].get_str();
  }
  aasr_topo *topo = nullptr;
  if (aasr_topo_create_from_ph(ph.c_str(), &topo) != AASR_OK) die(aasr_last_error());
  if (config["speakers"].specified) check_speakers(config["speakers"].get_str(), "lda");

  const std::string cfg = config["config"].get_str();
  std::ifstream cin_(cfg);
  if (!cin_) die("could not open " + cfg);
  std::stringstream ss;
  ss << cin_.rdbuf();

  const int device = config["device"].get_int();
  if (device >= 0 && aasr_set_device(device) != AASR_OK) die(aasr_last_error());

  aasr_lda_options opt;
  aasr_lda_default_options(&opt);
  opt.ophn = config["ophn"].specified;
  opt.info = config["info"].get_int();
  opt.target_dim = config["dim"].get_int();
  opt.maxmem = config["maxmem"].get_int();
  opt.no_silence = config["no-silence"].specified;
  opt.mingamma = config["mingamma"].get_double();
  opt.maxgamma = config["maxgamma"].get_double();
  const std::string module = config["module"].get_str(), speakers = config["speakers"].get_str(),
                    out = config["write-config"].get_str();
  opt.module = module.c_str();
  opt.speakers = config["speakers"].specified ? speakers.c_str() : nullptr;
  opt.out = config["write-config"].specified ? out.c_str() : nullptr;
  aasr_run_stats st;
  memset(&st, 0, sizeof st);
  if (networks) {
    // the remaining host-side refusals, before the model takes the device
    if (aasr_lda_networks_check(ss.str().c_str(), topo, config["recipe"].get_str().c_str(), &opt) != AASR_OK)
      die(aasr_last_error());
    aasr_gmm *gmm = nullptr;
    if (aasr_gmm_create_from_files(gk.c_str(), mc.c_str(), ph.c_str(), &gmm) != AASR_OK) die(aasr_last_error());
    aasr_lda_network_options nopt;
    aasr_lda_network_default_options(&nopt);
    nopt.networks = 1;
    nopt.viterbi = segmode == "vit";
    nopt.fw_beam = config["fw-beam"].get_float();
    nopt.bw_beam = config["bw-beam"].get_float();
    nopt.ac_scale_given = config["ac-scale"].specified;
    nopt.ac_scale = config["ac-scale"].get_float();
    if (aasr_run_lda_networks_recipe(ss.str().c_str(), gmm, topo, config["recipe"].get_str().c_str(), &opt, &nopt, &st) != AASR_OK)
      die(aasr_last_error());
    aasr_gmm_destroy(gmm);
    aasr_topo_destroy(topo);
    return 0;
  }
  // the remaining host-side refusals (-d against the module, the silence HMMs, recipe line limits) come first in there
  if (aasr_run_lda_recipe(ss.str().c_str(), topo, config["recipe"].get_str().c_str(), &opt, &st) != AASR_OK)
    die(aasr_last_error());
  aasr_topo_destroy(topo);
  return 0;
}
