// logl -- the log-likelihood of a recipe with the reference tool's options on the engine: per utterance the
// likelihood of its .phn state segmentation, or with -H / -D the forward-backward total over its HMM network, both on
// the device (aasr_run_logl_recipe); the reference's output on stdout.
//
//   logl (-b BASE | -g GK -m MC -p PH) -c CFG -r RECIPE [-O] [--snl] [-H | -D] [-F fw] [-W bw] [-A scale] [-V]
//        [-S SPKC] [-B n -I k] [-i level] [--device N]
//
// Refused before the device is opened: --mpv, a model file option missing, --batch without --bindex (or the reverse),
// non-diagonal and subspace pools, speaker files with model transforms, recipe start-line / end-line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "tool_common.hh"

int main(int argc, char *argv[]) {
  aku::conf::Config config;
  config("usage: logl [OPTION...]\n")
    ('h', "help", "", "", "display help")
    ('b', "base=BASENAME", "arg", "", "base filename for model files")
    ('g', "gk=FILE", "arg", "", "Mixture base distributions")
    ('m', "mc=FILE", "arg", "", "Mixture coefficients for the states")
    ('p', "ph=FILE", "arg", "", "HMM definitions")
    ('c', "config=FILE", "arg must", "", "feature configuration")
    ('r', "recipe=FILE", "arg must", "", "recipe file")
    ('O', "ophn", "", "", "use output phns for training")
    ('\0', "snl", "", "", "phn-files with state number labels")
    ('H', "hmmnet", "", "", "use HMM networks for training")
    ('D', "den-hmmnet", "", "", "use denominator HMM networks for training")
    ('F', "fw-beam=FLOAT", "arg", "0", "Forward beam (for HMM networks)")
    ('W', "bw-beam=FLOAT", "arg", "0", "Backward beam (for HMM networks)")
    ('A', "ac-scale=FLOAT", "arg", "1", "Acoustic scaling (for HMM networks)")
    ('M', "mpv", "", "", "Use Multipath Viterbi over HMM networks")
    ('V', "vit", "", "", "Use Viterbi over HMM networks")
    ('S', "speakers=FILE", "arg", "", "speaker configuration file")
    ('B', "batch=INT", "arg", "0", "number of batch processes with the same recipe")
    ('I', "bindex=INT", "arg", "0", "batch process index")
    ('i', "info=INT", "arg", "0", "info level")
    ('\0', "device=INT", "arg", "-1", "GPU ordinal (default: the first visible device)");
  config.default_parse(argc, argv);

  // the host's checks, in the tool's order of reading
  if (config["mpv"].specified)
    die("logl: --mpv (multipath Viterbi over the logical-arc hierarchy) is not supported; use -V or Baum-Welch");
  const std::string cfg = config["config"].get_str();
  std::ifstream cin_(cfg);
  if (!cin_) die("could not open " + cfg);
  std::stringstream ss;
  ss << cin_.rdbuf();
  std::string gk, mc, ph;
  resolve_model_files(config, &gk, &mc, &ph);
  if (config["batch"].specified != config["bindex"].specified) die("Must give both --batch and --bindex");
  check_pool(gk, "logl");
  if (config["speakers"].specified) check_speakers(config["speakers"].get_str(), "logl");
  const std::string recipe = config["recipe"].get_str();
  check_recipe_line_limits(recipe, config["batch"].get_int(), config["bindex"].get_int(), true, "logl");

  const int device = config["device"].get_int();
  if (device >= 0 && aasr_set_device(device) != AASR_OK) die(aasr_last_error());

  aasr_feat *feat = nullptr;
  aasr_gmm *gmm = nullptr;
  aasr_topo *topo = nullptr;
  if (aasr_feat_create(ss.str().c_str(), &feat) != AASR_OK) die(aasr_last_error());
  if (aasr_gmm_create_from_files(gk.c_str(), mc.c_str(), ph.c_str(), &gmm) != AASR_OK) die(aasr_last_error());
  if (aasr_topo_create_from_ph(ph.c_str(), &topo) != AASR_OK) die(aasr_last_error());
  aasr_spkc *spk = nullptr;
  if (config["speakers"].specified) {
    if (aasr_spkc_create(feat, gmm, &spk) != AASR_OK) die(aasr_last_error());
    if (aasr_spkc_read_file(spk, config["speakers"].get_str().c_str()) != AASR_OK) die(aasr_last_error());
  }

  aasr_logl_options opt;
  aasr_logl_default_options(&opt);
  opt.ophn = config["ophn"].specified;
  opt.snl = config["snl"].specified;
  opt.hmmnet = config["hmmnet"].specified;
  opt.den_hmmnet = config["den-hmmnet"].specified;
  opt.vit = config["vit"].specified;
  opt.fw_beam = config["fw-beam"].get_float();
  opt.bw_beam = config["bw-beam"].get_float();
  opt.ac_scale = config["ac-scale"].get_float();
  opt.ac_scale_given = config["ac-scale"].specified;
  opt.info = config["info"].get_int();
  opt.num_batches = config["batch"].get_int();
  opt.batch_index = config["bindex"].get_int();
  opt.speakers = spk;
  double total = 0;
  aasr_run_stats st;
  memset(&st, 0, sizeof st);
  if (aasr_run_logl_recipe(feat, gmm, topo, recipe.c_str(), &opt, &total, &st) != AASR_OK) die(aasr_last_error());
  fprintf(stdout, "Total log likelihood (%i/%i): %f\n", config["bindex"].get_int(), config["batch"].get_int(), total);
  if (spk) aasr_spkc_destroy(spk);
  aasr_topo_destroy(topo);
  aasr_gmm_destroy(gmm);
  aasr_feat_destroy(feat);
  return 0;
}
