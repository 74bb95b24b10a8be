// gcluster -- clustering of the Gaussian pool with the reference tool's options (aku/gcluster.cc:359-369) on the
// engine: random initial centres, Euclidean assignment, four passes of Kullback-Leibler assignment and centre
// re-estimation on the device (aasr_run_gcluster), the .gcl file that phone_probs -C reads.
//
//   gcluster -g FILE.gk -o FILE.gcl [-C clusters] [-t iterations] [-i level]
//
// Refused before the device is opened: -F (full-covariance centres), -R with -b (one group per regression class).
#include <string>

#include "tool_common.hh"

int main(int argc, char *argv[]) {
  aku::conf::Config config;
  config("usage: gcluster [OPTION...]\n")
    ('h', "help", "", "", "display help")
    ('g', "gk=FILE", "arg must", "", "gaussian definitions")
    ('o', "out=FILE", "arg must", "", "cluster file")
    ('F', "full", "", "", "use full statistics (much slower!) (not supported)")
    ('C', "clusters=INT", "arg", "1000", "number of clusters (default 1000)")
    ('t', "iterations=INT", "arg", "4", "number of iterations (default 4; without a regression tree four are made whatever is given, as in the reference)")
    ('R', "regtree=FILE", "arg", "", "regression tree file, if given, the clustering will group gaussians from the same treenode together (not supported)")
    ('b', "base=BASENAME", "arg", "", "base filename for model files, only necessary if regtree is given")
    ('i', "info=INT", "arg", "0", "info level")
    ('\0', "device=INT", "arg", "-1", "GPU ordinal (default: the first visible device)");
  config.default_parse(argc, argv);

  aasr_gcluster_options opt;
  aasr_gcluster_default_options(&opt);
  opt.info = config["info"].get_int();
  opt.clusters = config["clusters"].get_int();
  opt.iterations = config["iterations"].get_int();
  opt.full = config["full"].specified;
  opt.progress = 1;
  const std::string regtree = config["regtree"].get_str(), base = config["base"].get_str();
  opt.regtree = config["regtree"].specified ? regtree.c_str() : nullptr;
  opt.base = config["base"].specified ? base.c_str() : nullptr;

  const int device = config["device"].get_int();
  if (device >= 0 && aasr_set_device(device) != AASR_OK) die(aasr_last_error());
  // the pool is read and the options are checked in there, in the reference's order, before the device is opened
  if (aasr_run_gcluster(config["gk"].get_str().c_str(), config["out"].get_str().c_str(), &opt) != AASR_OK)
    die(aasr_last_error());
  return 0;
}
