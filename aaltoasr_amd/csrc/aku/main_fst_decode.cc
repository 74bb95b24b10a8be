// fst_decode -- words from a recipe: the FST token pass of the reference's FstSearch (decoder/src/FstSearch_tmpl.hh) on
// the device, a group of utterances per launch (aasr_run_fst_decode_recipe, csrc/fst_decode.cc).
//
//   fst_decode --fst FILE [--dur FILE [--dur-by-state]] [--beam F] [--token-limit N]
//              [--duration-scale F] [--transition-scale F] -r RECIPE -o OUT
//              ( (-b BASE | -g -m -p) -c CFG [-S SPKC] [--lnabytes 2|4]  |  --lna-files )
//              [--cap-candidates N] [--cap-recomb N] [--cap-history N]
//              [--confidence [--phone-loop FST [--phone-beam F] [--phone-token-limit N] [--phone-duration-scale F]]]
//              [-B n -I k] [-G utterances] [-i level] [--device N]
//
// --confidence: the reference's FstConfidence (with --phone-loop: FstConfidenceWithPhoneLoop, a second search over the
// phone-loop network on the same acoustics; aasr_run_fst_confidence_recipe).  A line is then
// `path logprob confidence words... [status]`, both numbers as %.9g; at -i 1 the reference's verbose block goes to stderr
// per utterance.  A --phone-* option without --confidence is refused.
// --lna-files: the recipe's lna= files (1-, 2- or 4-byte) are uploaded and searched -- what the reference's decoder does;
// no model and no feature configuration.  Engine mode: the recipe's audio= through the feature chain and the score + LNA
// step into the search, all on the device (--lnabytes 2 by default: precisely the values phone_probs would have
// written); no LNA file is written.  Output, one line per utterance: the recipe line's audio (engine mode) or lna path,
// the log-probability as %.9g, the words, and a trailing status word when the status is not OK.  Utterances that
// overflow a capacity (--cap-*: per utterance, 0 = derived) run once more with every capacity doubled; those that
// overflow again keep their OVERFLOW_* status.  Option errors are reported before the device is opened.
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
  config("usage: fst_decode [OPTION...]\n")
    ('h', "help", "", "", "display help")
    ('\0', "fst=FILE", "arg must", "", "search network (#FSTBasic MaxPlus)")
    ('\0', "dur=FILE", "arg", "", "duration model")
    ('\0', "dur-by-state", "", "", "index the duration tables by state (default: as the reference builds them)")
    ('\0', "beam=FLOAT", "arg", "2600", "beam")
    ('\0', "token-limit=INT", "arg", "5000", "token limit")
    ('\0', "duration-scale=FLOAT", "arg", "3", "duration scale")
    ('\0', "transition-scale=FLOAT", "arg", "1", "transition scale")
    ('r', "recipe=FILE", "arg must", "", "recipe file")
    ('o', "out=FILE", "arg must", "", "output file (- for stdout)")
    ('b', "base=BASENAME", "arg", "", "base filename for model files")
    ('g', "gk=FILE", "arg", "", "Mixture base distributions")
    ('m', "mc=FILE", "arg", "", "Mixture coefficients for the states")
    ('p', "ph=FILE", "arg", "", "HMM definitions")
    ('c', "config=FILE", "arg", "", "feature configuration")
    ('S', "speakers=FILE", "arg", "", "speaker configuration file")
    ('\0', "lnabytes=INT", "arg", "2", "engine mode: bytes per probability, 2 (default) or 4")
    ('\0', "lna-files", "", "", "search the recipe's lna= files")
    ('B', "batch=INT", "arg", "0", "number of batch processes with the same recipe")
    ('I', "bindex=INT", "arg", "0", "batch process index")
    ('G', "group=INT", "arg", "256", "utterances per launch")
    ('\0', "cap-candidates=INT", "arg", "0", "candidates per frame and utterance (0: derived)")
    ('\0', "cap-recomb=INT", "arg", "0", "recombination table entries, a power of two (0: derived)")
    ('\0', "cap-history=INT", "arg", "0", "history table entries, a power of two (0: derived)")
    ('\0', "confidence", "", "", "write a confidence in [0, 1] behind the log-probability")
    ('\0', "phone-loop=FILE", "arg", "", "phone-loop network of the confidence (#FSTBasic MaxPlus)")
    ('\0', "phone-beam=FLOAT", "arg", "2600", "beam of the phone-loop search")
    ('\0', "phone-token-limit=INT", "arg", "5000", "token limit of the phone-loop search")
    ('\0', "phone-duration-scale=FLOAT", "arg", "3", "duration scale of the phone-loop search")
    ('i', "info=INT", "arg", "0", "info level")
    ('\0', "device=INT", "arg", "-1", "GPU ordinal (default: the first visible device)");
  config.default_parse(argc, argv);

  // the host's checks
  const bool lna_files = config["lna-files"].specified;
  const bool model_opts = config["base"].specified || config["gk"].specified || config["mc"].specified || config["ph"].specified ||
                          config["config"].specified;
  if (lna_files && model_opts) die("fst_decode: --lna-files takes no model and no feature configuration");
  if (lna_files && config["lnabytes"].specified) die("fst_decode: --lnabytes belongs to engine mode; an LNA file states its own");
  if (lna_files && config["speakers"].specified) die("fst_decode: -S belongs to engine mode");
  const bool confidence = config["confidence"].specified;
  for (const char *name : {"phone-loop", "phone-beam", "phone-token-limit", "phone-duration-scale"}) {
    if (config[name].specified && !confidence) die(std::string("fst_decode: --") + name + " without --confidence");
    if (config[name].specified && !config["phone-loop"].specified) die(std::string("fst_decode: --") + name + " without --phone-loop");
  }
  if (config["dur-by-state"].specified && !config["dur"].specified) die("fst_decode: --dur-by-state without --dur");
  if (config["batch"].specified != config["bindex"].specified) die("Must give both --batch and --bindex");
  const int engine_bytes = config["lnabytes"].get_int();
  if (engine_bytes != 2 && engine_bytes != 4) die("Invalid number of LNA bytes");
  const int group_size = config["group"].get_int();
  if (group_size < 1) die("fst_decode: --group must be at least 1");
  aasr_fst_options opt;
  aasr_fst_default_options(&opt);
  opt.beam = config["beam"].get_float();
  opt.token_limit = config["token-limit"].get_int();
  opt.duration_scale = config["duration-scale"].get_float();
  opt.transition_scale = config["transition-scale"].get_float();
  opt.dur_by_state = config["dur-by-state"].specified;
  if (!(opt.beam >= 0)) die("fst_decode: the beam must not be negative");
  if (opt.token_limit < 0) die("fst_decode: the token limit must not be negative");
  opt.cap_candidates = config["cap-candidates"].get_int();
  opt.cap_recomb = config["cap-recomb"].get_int();
  opt.cap_history = config["cap-history"].get_int();
  if (opt.cap_candidates < 0 || opt.cap_recomb < 0 || opt.cap_history < 0) die("fst_decode: a capacity must not be negative");
  if ((opt.cap_recomb & (opt.cap_recomb - 1)) || (opt.cap_history & (opt.cap_history - 1)))
    die("fst_decode: --cap-recomb and --cap-history are powers of two");
  aasr_fst_options phone;
  aasr_fst_default_options(&phone);
  phone.beam = config["phone-beam"].get_float();
  phone.token_limit = config["phone-token-limit"].get_int();
  phone.duration_scale = config["phone-duration-scale"].get_float();
  phone.dur_by_state = opt.dur_by_state;
  if (!(phone.beam >= 0)) die("fst_decode: the phone beam must not be negative");
  if (phone.token_limit < 0) die("fst_decode: the phone token limit must not be negative");
  std::string gk, mc, ph, cfg_text;
  if (!lna_files) {
    if (!config["config"].specified) die("fst_decode: engine mode needs --config (or give --lna-files)");
    resolve_model_files(config, &gk, &mc, &ph);
    std::ifstream in(config["config"].get_str());
    if (!in) die("could not open " + config["config"].get_str());
    std::stringstream ss;
    ss << in.rdbuf();
    cfg_text = ss.str();
    check_pool(gk, "fst_decode");
    if (config["speakers"].specified) check_speakers(config["speakers"].get_str(), "fst_decode");
  }
  aasr_fstnet *net = nullptr;
  if (aasr_fstnet_create_from_file(config["fst"].get_str().c_str(), &net) != AASR_OK) die(std::string("fst_decode: ") + aasr_last_error());
  aasr_fstnet *phone_net = nullptr;
  if (config["phone-loop"].specified && aasr_fstnet_create_from_file(config["phone-loop"].get_str().c_str(), &phone_net) != AASR_OK)
    die(std::string("fst_decode: ") + aasr_last_error());
  aasr_fst_durations *dur = nullptr;
  if (config["dur"].specified && aasr_fst_durations_read(config["dur"].get_str().c_str(), &dur) != AASR_OK)
    die(std::string("fst_decode: ") + aasr_last_error());
  const std::vector<std::vector<std::string>> lines =
      recipe_lines(config["recipe"].get_str(), config["batch"].get_int(), config["bindex"].get_int(), false);
  for (const auto &fl : lines) {
    if (fl.size() != 13) die("fst_decode: malformed recipe line");
    if (lna_files && fl[6].empty()) die("fst_decode: --lna-files and a recipe line without lna=");
    if (!lna_files && fl[0].empty()) die("fst_decode: a recipe line without audio=");
  }

  const int device = config["device"].get_int();
  if (device >= 0 && aasr_set_device(device) != AASR_OK) die(aasr_last_error());
  aasr_feat *feat = nullptr;
  aasr_gmm *gmm = nullptr;
  aasr_spkc *spk = nullptr;
  if (!lna_files) {
    if (aasr_feat_create(cfg_text.c_str(), &feat) != AASR_OK) die(aasr_last_error());
    if (aasr_gmm_create_from_files(gk.c_str(), mc.c_str(), ph.c_str(), &gmm) != AASR_OK) die(aasr_last_error());
    if (config["speakers"].specified) {
      if (aasr_spkc_create(feat, gmm, &spk) != AASR_OK) die(aasr_last_error());
      if (aasr_spkc_read_file(spk, config["speakers"].get_str().c_str()) != AASR_OK) die(aasr_last_error());
    }
  }
  aasr_fst_decode_options run;
  aasr_fst_decode_default_options(&run);
  run.fst = opt;
  run.lna_files = lna_files;
  run.lnabytes = engine_bytes;
  run.group = group_size;
  run.num_batches = config["batch"].get_int();
  run.batch_index = config["bindex"].get_int();
  run.info = config["info"].get_int();
  run.speakers = spk;
  const std::string out_path = config["out"].get_str();
  run.out = out_path.c_str();
  aasr_run_stats st;
  memset(&st, 0, sizeof st);
  aasr_status status;
  if (confidence) {
    aasr_fst_confidence_options crun;
    aasr_fst_confidence_default_options(&crun);
    crun.decode = run;
    crun.phone = phone;
    crun.phone_loop = phone_net != nullptr;
    status = aasr_run_fst_confidence_recipe(feat, gmm, net, phone_net, dur, config["recipe"].get_str().c_str(), &crun, &st);
  } else {
    status = aasr_run_fst_decode_recipe(feat, gmm, net, dur, config["recipe"].get_str().c_str(), &run, &st);
  }
  if (status != AASR_OK) die(std::string("fst_decode: ") + aasr_last_error());
  if (run.info > 0)
    fprintf(stderr, "fst_decode: %lld utterances, %lld frames, %.3f s (%.3f s from upload to result)\n", (long long)st.utterances,
            (long long)st.frames, st.seconds_total, st.seconds_device);
  if (spk) aasr_spkc_destroy(spk);
  if (dur) aasr_fst_durations_destroy(dur);
  if (phone_net) aasr_fstnet_destroy(phone_net);
  aasr_fstnet_destroy(net);
  if (gmm) aasr_gmm_destroy(gmm);
  if (feat) aasr_feat_destroy(feat);
  return 0;
}
