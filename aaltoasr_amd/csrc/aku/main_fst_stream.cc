// fst_stream -- words while the speaker is still talking: headerless PCM16 on stdin through the feature chain, the
// score + LNA step and a streaming session of the FST token pass, a chunk of frames at a time, all on the device
// (aasr_run_fst_live, csrc/fst_live.cc; the reference's decoder/decode-stream.cc over its FstSearch).
//
//   fst_stream --fst FILE [--dur FILE [--dur-by-state]] (-b BASE | -g -m -p) -c CFG [--lnabytes 2|4]
//              [--beam F] [--token-limit N] [--duration-scale F] [--transition-scale F]
//              [--cap-candidates N] [--cap-recomb N] [--cap-history N]
//              [--confidence [--phone-loop FST [--phone-beam F] [--phone-token-limit N] [--phone-duration-scale F]]]
//              [--chunk-frames N] [--max-frames M] [--partial] [-i level] [--device N]      < PCM16
//
// The samples are read as frames become computable; a chunk of --chunk-frames frames (16) is searched as soon as its
// last frame is.  With --partial a line `frames logprob words...` is written and flushed whenever the best token's
// words differ from the ones printed last.  At the end of input one line in fst_decode's format with `-` as the path:
// `- logprob words... [STATUS]`, which is fst_decode's engine-mode line for the same samples whatever the chunk size.
// --max-frames (7500) bounds the input and sizes the search's tables; a longer input is refused when it gets there, and
// an utterance that overflows a capacity keeps its OVERFLOW_* status: the frames of a live stream are gone, nothing is
// rerun.  --confidence: a confidence behind every log-probability (aasr_run_fst_live_confidence: a streaming confidence
// session, with --phone-loop the reference's FstConfidenceWithPhoneLoop); the final line is then fst_decode --confidence's,
// `- logprob confidence words... [STATUS]`, and the --partial lines are `frames logprob confidence words...`.  A --phone-*
// option without --confidence is refused.  Option errors are reported before the device is opened.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "tool_common.hh"

int main(int argc, char *argv[]) {
  aku::conf::Config config;
  config("usage: fst_stream [OPTION...] < PCM16\n")
    ('h', "help", "", "", "display help")
    ('\0', "fst=FILE", "arg", "", "search network (#FSTBasic MaxPlus)")
    ('\0', "dur=FILE", "arg", "", "duration model")
    ('\0', "dur-by-state", "", "", "index the duration tables by state (default: as the reference builds them)")
    ('\0', "beam=FLOAT", "arg", "2600", "beam")
    ('\0', "token-limit=INT", "arg", "5000", "token limit")
    ('\0', "duration-scale=FLOAT", "arg", "3", "duration scale")
    ('\0', "transition-scale=FLOAT", "arg", "1", "transition scale")
    ('b', "base=BASENAME", "arg", "", "base filename for model files")
    ('g', "gk=FILE", "arg", "", "Mixture base distributions")
    ('m', "mc=FILE", "arg", "", "Mixture coefficients for the states")
    ('p', "ph=FILE", "arg", "", "HMM definitions")
    ('c', "config=FILE", "arg", "", "feature configuration")
    ('\0', "lnabytes=INT", "arg", "2", "bytes per probability, 2 (default) or 4")
    ('\0', "cap-candidates=INT", "arg", "0", "candidates per frame (0: derived)")
    ('\0', "cap-recomb=INT", "arg", "0", "recombination table entries, a power of two (0: derived)")
    ('\0', "cap-history=INT", "arg", "0", "history table entries, a power of two (0: derived)")
    ('\0', "chunk-frames=INT", "arg", "16", "frames per search launch")
    ('\0', "max-frames=INT", "arg", "7500", "the longest input, in frames")
    ('\0', "partial", "", "", "write the partial hypothesis whenever it changes")
    ('\0', "confidence", "", "", "write a confidence in [0, 1] behind the log-probability")
    ('\0', "phone-loop=FILE", "arg", "", "phone-loop network of the confidence (#FSTBasic MaxPlus)")
    ('\0', "phone-beam=FLOAT", "arg", "2600", "beam of the phone-loop search")
    ('\0', "phone-token-limit=INT", "arg", "5000", "token limit of the phone-loop search")
    ('\0', "phone-duration-scale=FLOAT", "arg", "3", "duration scale of the phone-loop search")
    ('i', "info=INT", "arg", "0", "info level")
    ('\0', "device=INT", "arg", "-1", "GPU ordinal (default: the first visible device)");
  config.default_parse(argc, argv);

  // the host's checks
  if (!config["fst"].specified) die("fst_stream: --fst is missing");
  if (!config["config"].specified) die("fst_stream: --config is missing");
  if (!config["base"].specified && !(config["gk"].specified && config["mc"].specified && config["ph"].specified))
    die("fst_stream: Must give either --base or all --gk, --mc and --ph");
  if (config["dur-by-state"].specified && !config["dur"].specified) die("fst_stream: --dur-by-state without --dur");
  const bool confidence = config["confidence"].specified;
  for (const char *name : {"phone-loop", "phone-beam", "phone-token-limit", "phone-duration-scale"}) {
    if (config[name].specified && !confidence) die(std::string("fst_stream: --") + name + " without --confidence");
    if (config[name].specified && !config["phone-loop"].specified) die(std::string("fst_stream: --") + name + " without --phone-loop");
  }
  aasr_fst_live_options run;
  aasr_fst_live_default_options(&run);
  run.lnabytes = config["lnabytes"].get_int();
  if (run.lnabytes != 2 && run.lnabytes != 4) die("fst_stream: --lnabytes is 2 or 4");
  run.chunk_frames = config["chunk-frames"].get_int();
  if (run.chunk_frames < 1) die("fst_stream: --chunk-frames must be at least 1");
  run.max_frames = config["max-frames"].get_int();
  if (run.max_frames < 1) die("fst_stream: --max-frames must be at least 1");
  aasr_fst_options &opt = run.fst;
  opt.beam = config["beam"].get_float();
  opt.token_limit = config["token-limit"].get_int();
  opt.duration_scale = config["duration-scale"].get_float();
  opt.transition_scale = config["transition-scale"].get_float();
  opt.dur_by_state = config["dur-by-state"].specified;
  if (!(opt.beam >= 0)) die("fst_stream: the beam must not be negative");
  if (opt.token_limit < 0) die("fst_stream: the token limit must not be negative");
  opt.cap_candidates = config["cap-candidates"].get_int();
  opt.cap_recomb = config["cap-recomb"].get_int();
  opt.cap_history = config["cap-history"].get_int();
  if (opt.cap_candidates < 0 || opt.cap_recomb < 0 || opt.cap_history < 0) die("fst_stream: a capacity must not be negative");
  if ((opt.cap_recomb & (opt.cap_recomb - 1)) || (opt.cap_history & (opt.cap_history - 1)))
    die("fst_stream: --cap-recomb and --cap-history are powers of two");
  aasr_fst_options phone;
  aasr_fst_default_options(&phone);
  phone.beam = config["phone-beam"].get_float();
  phone.token_limit = config["phone-token-limit"].get_int();
  phone.duration_scale = config["phone-duration-scale"].get_float();
  phone.dur_by_state = opt.dur_by_state;
  if (!(phone.beam >= 0)) die("fst_stream: the phone beam must not be negative");
  if (phone.token_limit < 0) die("fst_stream: the phone token limit must not be negative");
  run.partial = config["partial"].specified;
  run.info = config["info"].get_int();
  run.in_fd = 0;
  std::string gk, mc, ph;
  resolve_model_files(config, &gk, &mc, &ph);
  std::ifstream in(config["config"].get_str());
  if (!in) die("fst_stream: could not open " + config["config"].get_str());
  std::stringstream ss;
  ss << in.rdbuf();
  const std::string cfg_text = ss.str();
  check_pool(gk, "fst_stream");
  aasr_fstnet *net = nullptr;
  if (aasr_fstnet_create_from_file(config["fst"].get_str().c_str(), &net) != AASR_OK) die(std::string("fst_stream: ") + aasr_last_error());
  aasr_fstnet *phone_net = nullptr;
  if (config["phone-loop"].specified && aasr_fstnet_create_from_file(config["phone-loop"].get_str().c_str(), &phone_net) != AASR_OK)
    die(std::string("fst_stream: ") + aasr_last_error());
  aasr_fst_durations *dur = nullptr;
  if (config["dur"].specified && aasr_fst_durations_read(config["dur"].get_str().c_str(), &dur) != AASR_OK)
    die(std::string("fst_stream: ") + aasr_last_error());

  const int device = config["device"].get_int();
  if (device >= 0 && aasr_set_device(device) != AASR_OK) die(std::string("fst_stream: ") + aasr_last_error());
  aasr_feat *feat = nullptr;
  aasr_gmm *gmm = nullptr;
  if (aasr_feat_create(cfg_text.c_str(), &feat) != AASR_OK) die(std::string("fst_stream: ") + aasr_last_error());
  if (aasr_gmm_create_from_files(gk.c_str(), mc.c_str(), ph.c_str(), &gmm) != AASR_OK) die(std::string("fst_stream: ") + aasr_last_error());
  aasr_run_stats st;
  memset(&st, 0, sizeof st);
  aasr_status status;
  if (confidence) {
    aasr_fst_live_confidence_options crun;
    aasr_fst_live_confidence_default_options(&crun);
    crun.live = run;
    crun.phone = phone;
    crun.phone_loop = phone_net != nullptr;
    status = aasr_run_fst_live_confidence(feat, gmm, net, phone_net, dur, &crun, &st);
  } else {
    status = aasr_run_fst_live(feat, gmm, net, dur, &run, &st);
  }
  if (status != AASR_OK) die(std::string("fst_stream: ") + aasr_last_error());
  if (run.info > 0) fprintf(stderr, "fst_stream: %lld frames, %.3f s\n", (long long)st.frames, st.seconds_total);
  if (dur) aasr_fst_durations_destroy(dur);
  if (phone_net) aasr_fstnet_destroy(phone_net);
  aasr_fstnet_destroy(net);
  aasr_gmm_destroy(gmm);
  aasr_feat_destroy(feat);
  return 0;
}
