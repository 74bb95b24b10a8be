// vtln -- VTLN warp-factor estimation with the reference tool's options on the engine: per speaker a grid of warp
// factors, per grid point the utterances' features under that factor and the log-likelihood of their .phn state
// segmentations on the device (aasr_run_vtln_recipe), the best factor per speaker, the summary file and the speaker
// file as SpeakerConfig::write_speaker_file writes it.
//
//   vtln (-b BASE | -g GK -m MC -p PH) -c CFG -r RECIPE -v MODULE -S SPKC [-O] [-o OUT] [-s SUMMARY] [--snl] [--rsamp]
//        [--grid-size N] [--grid-rad R] [--relative] [-B n -I k] [-i level] [--device N]
//
// Refused before the device is opened: a model file option missing, --batch without --bindex (or the reverse), a
// module that the configuration does not give the type vtln, a recipe line without a speaker, recipe start-line /
// end-line, non-diagonal pools.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "tool_common.hh"

// the type of the module `name` in a feature configuration's text ("" when no module has the name): the "module { ... }"
// blocks' name and type entries, read as words
static std::string module_type(const std::string &cfg_text, const std::string &name) {
  std::istringstream in(cfg_text);
  std::vector<std::string> w;
  for (std::string t; in >> t;) w.push_back(t);
  for (size_t i = 0; i + 1 < w.size(); i++) {
    if (w[i] != "module" || w[i + 1] != "{") continue;
    std::string n, t;
    size_t j = i + 2;
    for (; j < w.size() && w[j] != "}"; j++) {
      if (w[j] == "name" && j + 1 < w.size()) n = w[j + 1];
      if (w[j] == "type" && j + 1 < w.size()) t = w[j + 1];
    }
    if (n == name) return t;
    i = j;
  }
  return "";
}

int main(int argc, char *argv[]) {
  aku::conf::Config config;
  config("usage: vtln [OPTION...]\n")
    ('h', "help", "", "", "display help")
    ('b', "base=BASENAME", "arg", "", "base filename for model files")
    ('g', "gk=FILE", "arg", "", "Gaussian kernels")
    ('m', "mc=FILE", "arg", "", "kernel indices for states")
    ('p', "ph=FILE", "arg", "", "HMM definitions")
    ('c', "config=FILE", "arg must", "", "feature configuration")
    ('r', "recipe=FILE", "arg must", "", "recipe file")
    ('O', "ophn", "", "", "use output phns for VTLN")
    ('v', "vtln=MODULE", "arg must", "", "VTLN module name")
    ('S', "speakers=FILE", "arg must", "", "speaker configuration input file")
    ('o', "out=FILE", "arg", "", "output speaker configuration file")
    ('s', "savesum=FILE", "arg", "", "save summary information (loglikelihoods)")
    ('\0', "snl", "", "", "phn-files with state number labels")
    ('\0', "rsamp", "", "", "phn sample numbers are relative to start time")
    ('\0', "grid-size=INT", "arg", "21", "warping grid size (default: 21/5)")
    ('\0', "grid-rad=FLOAT", "arg", "0.1", "radius of warping grid (default: 0.1/0.03)")
    ('\0', "relative", "", "", "relative warping grid (and smaller grid defaults)")
    ('B', "batch=INT", "arg", "0", "number of batch processes with the same recipe")
    ('I', "bindex=INT", "arg", "0", "batch process index")
    ('i', "info=INT", "arg", "0", "info level")
    ('\0', "device=INT", "arg", "-1", "GPU ordinal (default: the first visible device)");
  config.default_parse(argc, argv);

  // the host's checks, in the tool's order of reading: configuration, model files, batch options, recipe, module
  const std::string cfg = config["config"].get_str();
  std::ifstream cin_(cfg);
  if (!cin_) die("could not open " + cfg);
  std::stringstream ss;
  ss << cin_.rdbuf();
  std::string gk, mc, ph;
  resolve_model_files(config, &gk, &mc, &ph);
  if (config["batch"].specified != config["bindex"].specified) die("Must give both --batch and --bindex");
  check_pool(gk, "vtln");
  const std::string recipe = config["recipe"].get_str();
  check_recipe_line_limits(recipe, config["batch"].get_int(), config["bindex"].get_int(), true, "vtln");
  const std::string module = config["vtln"].get_str();
  {
    const std::string type = module_type(ss.str(), module);
    if (type.empty()) die("unknown module requested: " + module);
    if (type != "vtln") die("Module " + module + " is not a VTLN module");
  }
  {  // a line without a speaker (field 12 of 13 of the recipe table)
    std::ifstream rin(recipe);
    std::stringstream rs;
    rs << rin.rdbuf();
    char *table = nullptr;
    int64_t len = 0;
    if (aasr_recipe_read_all(rs.str().c_str(), config["batch"].get_int(), config["bindex"].get_int(), 1, &table, &len) != AASR_OK)
      die(aasr_last_error());
    std::istringstream lines(std::string(table, (size_t)len));
    aasr_free(table);
    for (std::string line; std::getline(lines, line);) {
      size_t at = 0;
      for (int k = 0; k < 11 && at != std::string::npos; k++) at = line.find('\x1f', at == 0 && k == 0 ? 0 : at + 1);
      if (at == std::string::npos) continue;
      const size_t end = line.find('\x1f', at + 1);
      if (line.substr(at + 1, end == std::string::npos ? std::string::npos : end - at - 1).empty()) die("Speaker ID is missing");
    }
  }

  const int device = config["device"].get_int();
  if (device >= 0 && aasr_set_device(device) != AASR_OK) die(aasr_last_error());

  aasr_feat *feat = nullptr;
  aasr_gmm *gmm = nullptr;
  aasr_topo *topo = nullptr;
  if (aasr_feat_create(ss.str().c_str(), &feat) != AASR_OK) die(aasr_last_error());
  if (aasr_gmm_create_from_files(gk.c_str(), mc.c_str(), ph.c_str(), &gmm) != AASR_OK) die(aasr_last_error());
  if (aasr_topo_create_from_ph(ph.c_str(), &topo) != AASR_OK) die(aasr_last_error());
  aasr_spkc *spk = nullptr;
  if (aasr_spkc_create(feat, gmm, &spk) != AASR_OK) die(aasr_last_error());
  if (aasr_spkc_read_file(spk, config["speakers"].get_str().c_str()) != AASR_OK) die(aasr_last_error());

  aasr_vtln_options opt;
  aasr_vtln_default_options(&opt);
  opt.ophn = config["ophn"].specified;
  opt.snl = config["snl"].specified;
  opt.rsamp = config["rsamp"].specified;
  opt.info = config["info"].get_int();
  opt.num_batches = config["batch"].get_int();
  opt.batch_index = config["bindex"].get_int();
  opt.grid_size = config["grid-size"].get_int();
  opt.grid_size_given = config["grid-size"].specified;
  opt.grid_rad = config["grid-rad"].get_float();
  opt.grid_rad_given = config["grid-rad"].specified;
  opt.relative = config["relative"].specified;
  const std::string out = config["out"].get_str(), savesum = config["savesum"].get_str();
  opt.module = module.c_str();
  opt.speakers = spk;
  opt.out = config["out"].specified ? out.c_str() : nullptr;
  opt.savesum = config["savesum"].specified ? savesum.c_str() : nullptr;
  aasr_run_stats st;
  memset(&st, 0, sizeof st);
  if (aasr_run_vtln_recipe(feat, gmm, topo, recipe.c_str(), &opt, &st) != AASR_OK) die(aasr_last_error());
  aasr_spkc_destroy(spk);
  aasr_topo_destroy(topo);
  aasr_gmm_destroy(gmm);
  aasr_feat_destroy(feat);
  return 0;
}
