// feanorm -- feature normalization and PCA estimation with the reference tool's options (aku/feanorm.cc:48-62) on the
// engine: the frames at the normalization module's source on the device, their blocked first and second moments
// there (the vector pipe; with --cov or -P the FP64 matrix pipe), the blocked sums, the mean and scale and the PCA on
// the host (aasr_run_feanorm_recipe).
//
//   feanorm -c CFG -r RECIPE [-M MODULE] [-P MODULE [-u]] [-w OUT.cfg] [-b BLOCK] [-S SPKC [--utt OUT.spkc]] [-p]
//           [--cov] [-i level]
//
// Refused before the device is opened: a -M module that is no normalization, a -P module that is no lin_transform or
// whose source has another dimension than the statistics, --utt without -M or without -S, speaker files with model
// transforms, more than 127 dimensions with --cov or -P.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "tool_common.hh"

int main(int argc, char *argv[]) {
  aku::conf::Config config;
  config("usage: feanorm [OPTION...]\n")
    ('h', "help", "", "", "display help")
    ('r', "recipe=FILE", "arg must", "", "recipe file")
    ('c', "config=FILE", "arg must", "", "read feature configuration")
    ('w', "write-config=FILE", "arg", "", "write feature configuration")
    ('M', "module=NAME", "arg", "", "normalization module name")
    ('P', "pca=NAME", "arg", "", "pca module name")
    ('u', "unit-determinant", "", "", "unit determinant for pca transform, by default unit variance for data")
    ('b', "block=INT", "arg", "1000", "block size (for reducing round-off errors)")
    ('\0', "utt=FILE", "arg", "", "estimate utterance normalization and write to a file")
    ('p', "print", "", "", "print mean and variance to stdout")
    ('\0', "cov", "", "", "estimate and print covariance matrix")
    ('S', "speakers=FILE", "arg", "", "speaker configuration file")
    ('i', "info=INT", "arg", "0", "info level")
    ('\0', "device=INT", "arg", "-1", "GPU ordinal (default: the first visible device)");
  config.default_parse(argc, argv);

  const std::string cfg = config["config"].get_str();
  std::ifstream cin_(cfg);
  if (!cin_) die("could not open " + cfg);
  std::stringstream ss;
  ss << cin_.rdbuf();
  if (config["speakers"].specified) check_speakers(config["speakers"].get_str(), "feanorm");

  const int device = config["device"].get_int();
  if (device >= 0 && aasr_set_device(device) != AASR_OK) die(aasr_last_error());

  aasr_feanorm_options opt;
  aasr_feanorm_default_options(&opt);
  opt.info = config["info"].get_int();
  opt.block_size = config["block"].get_int();
  opt.cov = config["cov"].specified;
  opt.print = config["print"].specified;
  opt.unit_determinant = config["unit-determinant"].specified;
  const std::string module = config["module"].get_str(), pca = config["pca"].get_str(), speakers = config["speakers"].get_str(),
                    utt = config["utt"].get_str(), out = config["write-config"].get_str();
  opt.module = config["module"].specified ? module.c_str() : nullptr;
  opt.pca = config["pca"].specified ? pca.c_str() : nullptr;
  opt.speakers = config["speakers"].specified ? speakers.c_str() : nullptr;
  opt.utt = config["utt"].specified ? utt.c_str() : nullptr;
  opt.out = config["write-config"].specified ? out.c_str() : nullptr;
  aasr_run_stats st;
  memset(&st, 0, sizeof st);
  // the reference's refusals (module types, --utt without -M or -S) come first in there, before the device
  if (aasr_run_feanorm_recipe(ss.str().c_str(), config["recipe"].get_str().c_str(), &opt, &st) != AASR_OK) die(aasr_last_error());
  return 0;
}
