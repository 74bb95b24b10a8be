// dur_est -- state duration models with the reference tool's options (aku/dur_est.cc:147-158): duration histograms and
// their gamma fits from state-numbered .phn files, such as stats --networks -M vit -a writes them, into the .dur file the
// decoder reads.  Host only (aasr_run_dur_est): no device is opened, and the tool runs where there is none.
//
//   dur_est -p PH -r RECIPE [-O] [-M maxdur] [--hist FILE] [--gamma FILE] [--skip n] [--mincount n] [-i level]
#include <string>

#include "tool_common.hh"

int main(int argc, char *argv[]) {
  aku::conf::Config config;
  config("usage: dur_est [OPTION...]\n")
    ('h', "help", "", "", "display help")
    ('p', "ph=FILE", "arg must", "", "HMM definitions")
    ('r', "recipe=FILE", "arg must", "", "recipe file")
    ('O', "ophn", "", "", "use output phns")
    ('M', "maxdur=INT", "arg", "100", "maximum duration noted (default 100)")
    ('\0', "hist=FILE", "arg", "", "write duration histograms to file")
    ('\0', "gamma=FILE", "arg", "", "write gamma models for durations to file")
    ('\0', "skip=INT", "arg", "0", "skip first INT states")
    ('\0', "mincount=INT", "arg", "10", "minimum occurance count to estimate gamma models")
    ('i', "info=INT", "arg", "0", "info level");
  config.default_parse(argc, argv);

  aasr_dur_est_options opt;
  aasr_dur_est_default_options(&opt);
  opt.ophn = config["ophn"].specified;
  opt.maxdur = config["maxdur"].get_int();
  opt.skip = config["skip"].get_int();
  opt.mincount = config["mincount"].get_int();
  opt.info = config["info"].get_int();
  const std::string hist = config["hist"].get_str(), gamma = config["gamma"].get_str();
  opt.hist = config["hist"].specified ? hist.c_str() : nullptr;
  opt.gamma = config["gamma"].specified ? gamma.c_str() : nullptr;
  if (aasr_run_dur_est(config["ph"].get_str().c_str(), config["recipe"].get_str().c_str(), &opt) != AASR_OK)
    die(aasr_last_error());
  return 0;
}
