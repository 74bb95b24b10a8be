// mllr -- constrained MLLR estimation with the reference tool's options (aku/mllr.cc:153-180) on the engine:
// features per utterance on the device under the speaker's current configuration, .phn segmentations on the
// host, the statistics of a speaker accumulated on the device (aasr_run_mllr_recipe), one solve per speaker,
// the speaker file as SpeakerConfig::write_speaker_file writes it.
//
//   mllr (-b BASE | -g GK -m MC -p PH) -c CFG -r RECIPE -S SPKC [-M MODULE] [-O] [-o OUT] [-B n -I k] [-i level]
//        [--networks [-F fw] [-W bw] [--segmode bw|vit]]
//
// Built: one global transform per speaker, for the lin_transform module -M names or (no -M) as a model-side
// cmllr block with unitmode UNIT_NO.  --networks is the reference's -H under a spelling of its own: Baum-Welch (or with
// --segmode vit Viterbi) over the recipe's hmmnet= networks on the device (aasr_run_mllr_networks_recipe), with -F / -W
// honoured; --segmode mpv and -O are refused with it, and a recipe line without hmmnet= is the reference's error.
// Refused before the device is opened: -H itself (use --networks), --segmode without --networks, -R and tree
// generation (-s with -t > 1), --snl, --rsamp, recipe start-line / end-line, non-diagonal pools.
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
  config("usage: modelmllr [OPTION...]\n")
    ('h', "help", "", "", "display help")
    ('b', "base=BASENAME", "arg", "", "base filename for model files")
    ('g', "gk=FILE", "arg", "", "Mixture base distributions")
    ('m', "mc=FILE", "arg", "", "Mixture coefficients for the states")
    ('p', "ph=FILE", "arg", "", "HMM definitions")
    ('c', "config=FILE", "arg must", "", "feature configuration")
    ('r', "recipe=FILE", "arg must", "", "recipe file")
    ('O', "ophn", "", "", "use output phns for adaptation")
    ('H', "hmmnet", "", "", "use HMM networks for training")
    ('\0', "segmode=MODE", "arg", "bw", "Segmentation mode: bw(default)/vit/mpv")
    ('M', "mllr=MODULE", "arg", "", "MLLR feature module name, if none given, a model transform is trained. Only for a model transform the regression tree options are used.")
    ('S', "speakers=FILE", "arg must", "", "speaker configuration input file")
    ('R', "regtree=FILE", "arg", "", "regression tree file, if ommitted, and the next tree options are given, a tree is generated. Otherwise no tree is used.")
    ('s', "mcs=FILE", "arg", "", "Mixture statistics file (necessary for generating a tree, if no tree file is given)")
    ('t', "terminalnodes=INT", "arg", "1", "Number of maximum terminal nodes (used for generating a tree, if no tree file is given)")
    ('u', "unit=STRING", "arg", "PHONE", "PHONE|MIX|GAUSSIAN type of units. Don't use MIX in case of shared gaussians between mixtures (used for generating a tree, if no tree file is given)")
    ('f', "minframes=DOUBLE", "arg", "1000", "minimum frames used for adaptation")
    ('o', "out=FILE", "arg", "", "output speaker configuration file")
    ('F', "fw-beam=FLOAT", "arg", "0", "Forward beam (for HMM networks)")
    ('W', "bw-beam=FLOAT", "arg", "0", "Backward beam (for HMM networks)")
    ('\0', "snl", "", "", "phn-files with state number labels")
    ('\0', "rsamp", "", "", "phn sample numbers are relative to start time")
    ('\0', "ords","", "", "OBSOLETE, does not have any function anymore")
    ('B', "batch=INT", "arg", "0", "number of batch processes with the same recipe")
    ('I', "bindex=INT", "arg", "0", "batch process index")
    ('i', "info=INT", "arg", "0", "info level")
    ('\0', "device=INT", "arg", "-1", "GPU ordinal (default: the first visible device)")
    ('\0', "networks", "", "", "segment with the recipe's hmmnet= networks; the reference's -H");
  config.default_parse(argc, argv);

  if (config["ords"].specified)
    fprintf(stderr, "Warning: --ords is obsolete and does not have to be used anymore\n");

  // what this build does not do, refused before anything is read
  const char *refused[][2] = {{"hmmnet", "-H (HMM network segmentation)"},
                              {"segmode", "--segmode (HMM network segmentation)"},
                              {"regtree", "-R (regression tree)"},
                              {"snl", "--snl (state number labels)"},
                              {"rsamp", "--rsamp (relative sample numbers)"}};
  const bool networks = config["networks"].specified;
  for (const auto &r : refused) {
    if (networks && std::string(r[0]) == "segmode") continue;
    if (config[r[0]].specified)
      die(std::string("mllr: ") + r[1] + " is not supported; only global transforms over .phn files are" +
          (std::string(r[0]) == "hmmnet" ? ", and over HMM networks with --networks" : ""));
  }
  const std::string segmode = config["segmode"].get_str();
  if (networks) {
    if (segmode == "mpv")
      die("mllr: --segmode mpv (multipath Viterbi) is not supported with --networks; use --segmode bw or --segmode vit");
    if (segmode != "bw" && segmode != "vit") die("Invalid segmentation mode " + segmode);  // aku/mllr.cc:208-210
    if (config["ophn"].specified) die("mllr: -O (output phns) is not supported with --networks");
  }
  const bool global_transform = config["mllr"].specified;
  if (config["mcs"].specified && config["terminalnodes"].get_int() > 1 && !global_transform) {
    // the reference checks the unit before it builds the tree (aku/mllr.cc:238-242)
    const std::string unit = config["unit"].get_str();
    if (unit != "PHONE" && unit != "MIX" && unit != "GAUSSIAN") die(unit + " is not a valid unit identifier");
    die("mllr: tree generation (-s with -t > 1) is not supported; only global transforms over .phn files are");
  }

  std::string gk, mc, ph;
  resolve_model_files(config, &gk, &mc, &ph);
  check_pool(gk, "mllr");
  check_recipe_line_limits(config["recipe"].get_str(), config["batch"].get_int(), config["bindex"].get_int(), true,
                           "mllr");
  if (networks)
    check_recipe_hmmnets(config["recipe"].get_str(), config["batch"].get_int(), config["bindex"].get_int(), true);

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
  const int info = config["info"].get_int();
  if (!global_transform && info > 0) fprintf(stderr, "No regression tree used\n");

  aasr_spkc *spk = nullptr;
  if (aasr_spkc_create(feat, gmm, &spk) != AASR_OK) die(aasr_last_error());
  if (aasr_spkc_read_file(spk, config["speakers"].get_str().c_str()) != AASR_OK) die(aasr_last_error());

  aasr_mllr_options opt;
  aasr_mllr_default_options(&opt);
  opt.ophn = config["ophn"].specified;
  opt.info = info;
  opt.num_batches = config["batch"].get_int();
  opt.batch_index = config["bindex"].get_int();
  opt.minframes = config["minframes"].get_double();
  const std::string module = config["mllr"].get_str(), out = config["out"].get_str();
  opt.module = global_transform ? module.c_str() : nullptr;
  opt.speakers = spk;
  opt.out = config["out"].specified ? out.c_str() : nullptr;
  aasr_run_stats st;
  memset(&st, 0, sizeof st);
  aasr_mllr_network_options nopt;
  aasr_mllr_network_default_options(&nopt);
  nopt.networks = networks;
  nopt.viterbi = segmode == "vit";
  nopt.fw_beam = config["fw-beam"].get_float();
  nopt.bw_beam = config["bw-beam"].get_float();
  if (aasr_run_mllr_networks_recipe(feat, gmm, topo, config["recipe"].get_str().c_str(), &opt, &nopt, &st) != AASR_OK)
    die(aasr_last_error());
  aasr_spkc_destroy(spk);
  aasr_topo_destroy(topo);
  aasr_gmm_destroy(gmm);
  aasr_feat_destroy(feat);
  return 0;
}
