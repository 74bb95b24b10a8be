// tie -- decision-tree state tying with the reference tool's options (aku/tie.cc:115-136) on the engine: the context
// phones of the recipe's state-numbered .phn files, their full-covariance statistics on the FP64 matrix pipe, the
// split search and the merge on the device (aasr_run_tie_recipe), a basebind file or a model with one full-covariance
// Gaussian per tied state.
//
//   tie -c CFG -r RECIPE -u RULES (-o BASE | -B BASEBIND) [-O] [--count N] [--sgain G] [--mloss L] [--context N]
//       [-S SPKC] [-i level]
//
// -H gives the reference's own message ("This feature is currently broken. Fix it?") before anything is read;
// -b -C -F -W -A -V belong to it and are parsed only.  Refused before the device is opened: neither or both of -o and
// -B, recipe start-line / end-line, speaker files with model transforms, a bad rule file, a .phn line without a
// state number.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "tool_common.hh"

int main(int argc, char *argv[]) {
  aku::conf::Config config;
  config("usage: tie [OPTION...]\n")
    ('h', "help", "", "", "display help")
    ('c', "config=FILE", "arg must", "", "feature configuration")
    ('r', "recipe=FILE", "arg must", "", "recipe file")
    ('O', "ophn", "", "", "use output phns for training")
    ('H', "hmmnet", "", "", "use HMM networks for training")
    ('b', "base=BASENAME", "arg", "", "model files (required with --hmmnet)")
    ('C', "mconfig=FILE", "arg", "", "model configuration (optional)")
    ('u', "rule=FILE", "arg must", "", "rule set for triphone state tying")
    ('o', "out=FILE", "arg", "", "write output to HMM model with base name FILE")
    ('B', "basebind=FILE", "arg", "", "write output to basebind FILE")
    ('\0', "count=INT", "arg", "100", "minimum feature count for state clusters")
    ('\0', "sgain=FLOAT", "arg", "0", "minimum loglikelihood gain in cluster splitting")
    ('\0', "mloss=FLOAT", "arg", "0", "cluster merging with maximum loglikelihood loss")
    ('\0', "context=INT", "arg", "1", "maximum number of contexts (default 1=triphones)")
    ('F', "fw-beam=FLOAT", "arg", "0", "Forward beam (for HMM networks)")
    ('W', "bw-beam=FLOAT", "arg", "0", "Backward beam (for HMM networks)")
    ('A', "ac-scale=FLOAT", "arg", "1", "Acoustic scaling (for HMM networks)")
    ('V', "vit", "", "", "Use Viterbi over HMM networks")
    ('S', "speakers=FILE", "arg", "", "speaker configuration file")
    ('i', "info=INT", "arg", "0", "info level")
    ('\0', "device=INT", "arg", "-1", "GPU ordinal (default: the first visible device)");
  config.default_parse(argc, argv);

  if (config["hmmnet"].specified) die("This feature is currently broken. Fix it?");
  if (!(config["out"].specified ^ config["basebind"].specified)) die("Specify either --out or --basebind for output");
  if (config["speakers"].specified) check_speakers(config["speakers"].get_str(), "tie");

  const std::string cfg = config["config"].get_str();
  std::ifstream cin_(cfg);
  if (!cin_) die("could not open " + cfg);
  std::stringstream ss;
  ss << cin_.rdbuf();

  const int device = config["device"].get_int();
  if (device >= 0 && aasr_set_device(device) != AASR_OK) die(aasr_last_error());

  aasr_tie_options opt;
  aasr_tie_default_options(&opt);
  opt.ophn = config["ophn"].specified;
  opt.info = config["info"].get_int();
  opt.count = config["count"].get_int();
  opt.context = config["context"].get_int();
  // set_clustering_parameters takes the reference's get_float() values as doubles
  opt.sgain = (double)config["sgain"].get_float();
  opt.mloss = (double)config["mloss"].get_float();
  opt.mloss_given = config["mloss"].specified;
  const std::string rule = config["rule"].get_str(), speakers = config["speakers"].get_str(), out = config["out"].get_str(),
                    basebind = config["basebind"].get_str();
  opt.rule = rule.c_str();
  opt.speakers = config["speakers"].specified ? speakers.c_str() : nullptr;
  opt.out = config["out"].specified ? out.c_str() : nullptr;
  opt.basebind = config["basebind"].specified ? basebind.c_str() : nullptr;
  aasr_run_stats st;
  memset(&st, 0, sizeof st);
  if (aasr_run_tie_recipe(ss.str().c_str(), config["recipe"].get_str().c_str(), &opt, &st) != AASR_OK) die(aasr_last_error());
  return 0;
}
