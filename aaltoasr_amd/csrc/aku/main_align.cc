// align -- forced alignment with the reference tool's options and defaults (aku/align.cc:180-198)
// on the engine: features and scores per utterance, the Viterbi search on the device for many
// utterances at once (aasr_run_align_recipe), .phn files as align writes them.
//
//   align (-b BASE | -g GK -m MC -p PH) -c CFG -r RECIPE [--swins N] [--beam F] [--sbeam N]
//         [--maxbeam F] [--overlap F] [--no-force-end] [--phoseg] [-S SPKC] [-B n -I k] [-i level]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "tool_common.hh"

int main(int argc, char *argv[]) {
  aku::conf::Config config;
  config("usage: align [OPTION...]\n")
    ('h', "help", "", "", "display help")
    ('b', "base=BASENAME", "arg", "", "base filename for model files")
    ('g', "gk=FILE", "arg", "", "Gaussian kernels")
    ('m', "mc=FILE", "arg", "", "kernel indices for states")
    ('p', "ph=FILE", "arg", "", "HMM definitions")
    ('c', "config=FILE", "arg must", "", "feature configuration")
    ('r', "recipe=FILE", "arg must", "", "recipe file")
    ('\0', "swins=INT", "arg", "1000", "window size (default: 1000)")
    ('\0', "beam=FLOAT", "arg", "100.0", "log prob beam (default 100.0)")
    ('\0', "sbeam=INT", "arg", "100", "state beam (default 100)")
    ('\0', "maxbeam=FLOAT", "arg", "1600.0", "max beam for retries (default 1600.0)")
    ('\0', "overlap=FLOAT", "arg", "0.4", "Viterbi window overlap (default 0.4)")
    ('\0', "no-force-end", "", "", "do not force to the last state")
    ('\0', "phoseg", "", "", "print phoneme segmentation instead of states")
    ('S', "speakers=FILE", "arg", "", "speaker configuration file")
    ('B', "batch=INT", "arg", "0", "number of batch processes with the same recipe")
    ('I', "bindex=INT", "arg", "0", "batch process index")
    ('i', "info=INT", "arg", "0", "info level")
    ('\0', "device=INT", "arg", "-1", "GPU ordinal (default: the first visible device)");
  config.default_parse(argc, argv);

  std::string gk, mc, ph;
  resolve_model_files(config, &gk, &mc, &ph);
  const int device = config["device"].get_int();
  if (device >= 0 && aasr_set_device(device) != AASR_OK) die(aasr_last_error());

  // the topology and the options need no device: an empty batch checks the options before any model is loaded
  aasr_topo *topo = nullptr;
  if (aasr_topo_create_from_ph(ph.c_str(), &topo) != AASR_OK) die(aasr_last_error());
  aasr_align_options opt;
  aasr_align_default_options(&opt);
  opt.swins = config["swins"].get_int();
  opt.beam = config["beam"].get_float();
  opt.sbeam = config["sbeam"].get_int();
  opt.maxbeam = config["maxbeam"].get_float();
  opt.overlap = config["overlap"].get_float();
  opt.no_force_end = config["no-force-end"].specified;
  opt.phoseg = config["phoseg"].specified;
  opt.info = config["info"].get_int();
  opt.num_batches = config["batch"].get_int();
  opt.batch_index = config["bindex"].get_int();
  {
    aasr_align_batch *none = nullptr;
    if (aasr_align_batch_create(topo, &opt, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &none) != AASR_OK)
      die(aasr_last_error());
    aasr_align_batch_destroy(none);
  }

  const std::string cfg = config["config"].get_str();
  std::ifstream cin_(cfg);
  if (!cin_) die("could not open " + cfg);
  std::stringstream ss;
  ss << cin_.rdbuf();
  aasr_feat *feat = nullptr;
  aasr_gmm *gmm = nullptr;
  if (aasr_feat_create(ss.str().c_str(), &feat) != AASR_OK) die(aasr_last_error());
  if (aasr_gmm_create_from_files(gk.c_str(), mc.c_str(), ph.c_str(), &gmm) != AASR_OK) die(aasr_last_error());

  aasr_spkc *spk = nullptr;
  if (config["speakers"].specified) {
    if (aasr_spkc_create(feat, gmm, &spk) != AASR_OK) die(aasr_last_error());
    if (aasr_spkc_read_file(spk, config["speakers"].get_str().c_str()) != AASR_OK) die(aasr_last_error());
  }
  opt.speakers = spk;
  aasr_run_stats st;
  memset(&st, 0, sizeof st);
  if (aasr_run_align_recipe(feat, gmm, topo, config["recipe"].get_str().c_str(), &opt, &st) != AASR_OK)
    die(aasr_last_error());
  aasr_spkc_destroy(spk);
  aasr_topo_destroy(topo);
  aasr_gmm_destroy(gmm);
  aasr_feat_destroy(feat);
  return 0;
}
