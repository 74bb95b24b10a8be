// tool_common.hh -- what the command-line tools (main_*.cc) share: the fatal message, the model file options and the
// refusals a tool makes on the host before the device is opened.  Header only: every tool is one source file on the
// public ABI.
#ifndef AKU_AMD_TOOL_COMMON_HH
#define AKU_AMD_TOOL_COMMON_HH

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/aasr.h"
#include "conf.hh"

[[noreturn]] static inline void die(const std::string &msg) {
  fprintf(stderr, "exception: %s\n", msg.c_str());
  exit(1);
}

// --base BASENAME, or all of --gk, --mc and --ph
static inline void resolve_model_files(aku::conf::Config &config, std::string *gk, std::string *mc, std::string *ph) {
  if (config["base"].specified) {
    const std::string base = config["base"].get_str();
    *gk = base + ".gk";
    *mc = base + ".mc";
    *ph = base + ".ph";
  } else if (config["gk"].specified && config["mc"].specified && config["ph"].specified) {
    *gk = config["gk"].get_str();
    *mc = config["mc"].get_str();
    *ph = config["ph"].get_str();
  } else {
    die("Must give either --base or all --gk, --mc and --ph");
  }
}

// PDFPool::read_gk's header and per-Gaussian tags, without the values: diagonal pools only
static inline void check_pool(const std::string &gk, const std::string &tool) {
  std::ifstream in(gk);
  if (!in) die("could not open " + gk);
  int size = 0, dim = 0;
  std::string kind;
  in >> size >> dim >> kind;
  if (!in) die("could not read the header of " + gk);
  if (kind == "diagonal_cov") return;
  if (kind != "variable") die(tool + ": only diagonal Gaussians are supported (" + gk + " is a " + kind + " pool)");
  std::string tag, value;
  for (int g = 0; g < size; g++) {
    if (!(in >> tag)) die("could not read " + gk);
    if (tag != "diag") die(tool + ": only diagonal Gaussians are supported (" + gk + " holds '" + tag + "' Gaussians)");
    for (int i = 0; i < 2 * dim; i++) in >> value;
  }
}

// a speaker file's "model <module>" entries set model-side transforms (ModelTransformer)
static inline void check_speakers(const std::string &path, const std::string &tool) {
  std::ifstream in(path);
  if (!in) die("could not open " + path);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string first;
    if (ls >> first && first == "model")
      die(tool + ": speaker files with model transforms (" + line + ") are not supported");
  }
}

// the recipe's lines of this batch as aasr_recipe_read_all gives them: 13 fields a line
static inline std::vector<std::vector<std::string>> recipe_lines(const std::string &path, int num_batches, int batch_index,
                                                                 bool cluster_speakers) {
  std::ifstream in(path);
  if (!in) die("could not open " + path);
  std::stringstream ss;
  ss << in.rdbuf();
  char *table = nullptr;
  int64_t len = 0;
  if (aasr_recipe_read_all(ss.str().c_str(), num_batches, batch_index, cluster_speakers ? 1 : 0, &table, &len) != AASR_OK)
    die(aasr_last_error());
  const std::string t(table, (size_t)len);
  aasr_free(table);
  std::vector<std::vector<std::string>> out;
  std::istringstream lines(t);
  std::string line;
  while (std::getline(lines, line)) {
    std::vector<std::string> fl;
    size_t a = 0;
    for (;;) {
      const size_t b = line.find('\x1f', a);
      fl.push_back(line.substr(a, b == std::string::npos ? std::string::npos : b - a));
      if (b == std::string::npos) break;
      a = b + 1;
    }
    out.push_back(fl);
  }
  return out;
}

// recipe lines with start-line / end-line, refused as the drivers refuse them
static inline void check_recipe_line_limits(const std::string &path, int num_batches, int batch_index,
                                            bool cluster_speakers, const std::string &tool) {
  for (const std::vector<std::string> &fl : recipe_lines(path, num_batches, batch_index, cluster_speakers))
    if (fl.size() == 13 && (atoi(fl[9].c_str()) > 0 || atoi(fl[10].c_str()) > 0))
      die(tool + ": recipe line limits (start-line / end-line) are not supported");
}

// a network tool's recipe: every line names its hmmnet= file (Recipe::Info::init_hmmnet_files, Recipe.cc:198-231)
static inline void check_recipe_hmmnets(const std::string &path, int num_batches, int batch_index, bool cluster_speakers) {
  for (const std::vector<std::string> &fl : recipe_lines(path, num_batches, batch_index, cluster_speakers))
    if (fl.size() == 13 && fl[4].empty()) die("Recipe::Info::init_hmmnet_files: hmmnet not specified in recipe.");
}

#endif
