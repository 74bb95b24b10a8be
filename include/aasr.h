/*
 * aasr.h -- C ABI of the MI355X-native acoustic-likelihood engine.
 *
 * Drop-in boundary for AaltoASR's frame-parallel hot path
 *     16 kHz PCM -> MFCC chain -> diagonal-GMM state likelihoods -> LNA
 * i.e. what aku/phone_probs.cc and aku/PhoneProbsToolbox.cc drive through
 * aku::FeatureGenerator and aku::HmmSet.  Plain pointers and sizes only; no
 * C++/torch types.  Each entry point cites the reference interface it
 * replaces (paths relative to the AaltoASR tree).
 *
 * Conventions
 *  - Every function returns AASR_OK (0) or a negative aasr_status; the message
 *    is available from aasr_last_error() (thread-local).  Nothing throws
 *    across this boundary.  The C++ adapters in aaltoasr_amd/csrc/aku/ rethrow
 *    as std::string / HmmSet::*Error exactly where the reference throws.
 *  - Handles own their device memory.  Caller owns every host buffer.
 *  - "_dev" variants take device pointers (hipMalloc'ed / torch tensors) and a
 *    hipStream_t passed as void*; they enqueue work and do not synchronise.
 *    Host variants copy in, run, copy out, and synchronise.
 *  - A handle is bound to the HIP device current at creation; handles are not
 *    thread-safe, distinct handles are independent.
 *  - There is NO CPU fallback: without a usable HIP device the compute entry
 *    points return AASR_ERR_NO_DEVICE.
 */
#ifndef AASR_H
#define AASR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int aasr_status;
enum {
  AASR_OK = 0,
  AASR_ERR_INVALID = -1,     /* bad argument / malformed config or model      */
  AASR_ERR_UNSUPPORTED = -2, /* valid for the reference, not built here (loud) */
  AASR_ERR_NO_DEVICE = -3,   /* no HIP device / HIP runtime error              */
  AASR_ERR_IO = -4,          /* file open/read/write failure                   */
  AASR_ERR_SHORT_AUDIO = -5  /* "audio shorter than frame" FeatureModules.cc:409 */
};

typedef struct aasr_feat aasr_feat;   /* compiled feature graph (.cfg)  */
typedef struct aasr_gmm aasr_gmm;     /* acoustic model resident in HBM */

const char *aasr_last_error(void);
const char *aasr_version(void);
/* number of visible HIP devices (0 when none / no driver) */
int aasr_device_count(void);
aasr_status aasr_set_device(int ordinal);

/* ------------------------------------------------------------------------ */
/* Feature chain: replaces aku::FeatureGenerator + FeatureModule::generate  */
/* ------------------------------------------------------------------------ */

/* FeatureGenerator::load_configuration (aku/FeatureGenerator.cc:96-219):
 * cfg_text is the text of a feature configuration file ("module { ... }"
 * blocks, aku/ModuleConfig.cc:166-202).  Supported module types: audiofile,
 * fft, mel, power, dct, delta, normalization, lin_transform, merge,
 * mean_subtractor; any other reference type -> AASR_ERR_UNSUPPORTED, unknown
 * type -> AASR_ERR_INVALID ("Unknown module type"). */
aasr_status aasr_feat_create(const char *cfg_text, aasr_feat **out);
void aasr_feat_destroy(aasr_feat *h);

/* FeatureGenerator::dim / frame_rate / sample_rate
 * (aku/FeatureGenerator.cc:281-300) */
int aasr_feat_dim(const aasr_feat *h);
float aasr_feat_frame_rate(const aasr_feat *h);
int aasr_feat_sample_rate(const aasr_feat *h);
/* dim of a named module (FeatureGenerator::module(name)->dim()), -1 unknown */
int aasr_feat_module_dim(const aasr_feat *h, const char *module_name);
/* base-module frames of look-around one output frame needs (left, right):
 * the sum of DeltaModule / MeanSubtractorModule offsets along the graph
 * (aku/FeatureModules.cc:1014-1015, 1390-1400), plus 7 frames on the left per
 * mean subtractor: its kernel anchors the window sum on frame numbers that are
 * multiples of 8 and slides it from there, so it reads up to 7 rows before the window */
void aasr_feat_halo(const aasr_feat *h, int *left, int *right);

/* AudioFileModule::last_frame (aku/FeatureModules.cc:305-308) for a file of
 * n_samples; the whole-file frame count phone_probs emits is last_frame+1
 * (aku/phone_probs.cc:217-221). */
int aasr_feat_last_frame(const aasr_feat *h, int64_t n_samples);
/* The frame at which a sequential reader of n_samples meets the end: the first frame whose window
 * crosses it (AudioFileModule::generate, aku/FeatureModules.cc:399-413 sets m_eof_frame there).
 * phone_probs emits frames 0 .. eof_frame - 1 and the border copy repeats frame eof_frame - 1.
 * Equal to last_frame() + 1 except where last_frame()'s float formula is off by one (inputs
 * beyond 2^24 samples, fractional window advances). */
int aasr_feat_eof_frame(const aasr_feat *h, int64_t n_samples);

/* Graphs whose first module is a `pre` module (PreModule,
 * aku/FeatureModules.cc:572-755) take float feature frames instead of audio:
 * what `feacat --raw-output -H` writes (int32 dimension, then float32 frames;
 * legacy_file 1: a one-byte dimension).  Frames before 0 repeat frame 0, frames
 * past the end repeat the last one.  n_values = frames x input dimension.
 * aasr_feat_last_frame and the batch entry points count such input in int16
 * units (2 per float) so that audio and feature input share every buffer. */
aasr_status aasr_feat_run_features(aasr_feat *h, const float *features, int64_t n_values,
                                   int32_t first_frame, int32_t n_frames,
                                   const char *module_name, float *out);
aasr_status aasr_feat_run_features_f64(aasr_feat *h, const float *features, int64_t n_values,
                                       int32_t first_frame, int32_t n_frames,
                                       const char *module_name, double *out);
/* FeatureGenerator::write_configuration (aku/FeatureGenerator.cc:222-243): the graph as .cfg text in
 * the reference's own layout (every option a module saves, "%g" / "%d" values, "sources" last), so
 * that re-reading it rebuilds the same graph.  *text is malloc'ed; free it with aasr_free. */
aasr_status aasr_feat_write_config(const aasr_feat *h, char **text, int64_t *len);
int aasr_feat_input_is_features(const aasr_feat *h);   /* 1 when the base module is `pre` */
int aasr_feat_pre_legacy(const aasr_feat *h);          /* its legacy_file option */
int aasr_feat_input_dim(const aasr_feat *h);           /* dimension of the base module */

/* FeatureGenerator::generate(frame) for frames first_frame ..
 * first_frame+n_frames-1 of one utterance whose complete PCM (mono int16,
 * what AudioReader::fetch delivers, aku/AudioReader.cc:219-230) is pcm[0..
 * n_samples).  Negative frames and frames past EOF follow copy_borders
 * (aku/FeatureModules.cc:381-397).  out is float32 [n_frames x dim].
 * module_name NULL = last module (the generator's output). */
aasr_status aasr_feat_run(aasr_feat *h, const int16_t *pcm, int64_t n_samples,
                          int32_t first_frame, int32_t n_frames,
                          const char *module_name, float *out);
aasr_status aasr_feat_run_dev(aasr_feat *h, const int16_t *d_pcm,
                              int64_t n_samples, int32_t first_frame,
                              int32_t n_frames, float *d_out, void *stream);
/* double-precision output of the same frames (the reference's FeatureVec is
 * double, aku/FeatureBuffer.hh:15-89); used by the adapters and parity tests */
aasr_status aasr_feat_run_f64(aasr_feat *h, const int16_t *pcm,
                              int64_t n_samples, int32_t first_frame,
                              int32_t n_frames, const char *module_name,
                              double *out);

/* The double-precision frames of aasr_feat_run_f64 written to device memory: d_pcm holds the
 * utterance's complete input on the device (int16 units, as aasr_feat_run_dev), d_out receives
 * [n_frames x dim] doubles.  Enqueued on `stream`, no host wait. */
aasr_status aasr_feat_run_f64_dev(aasr_feat *h, const int16_t *d_pcm, int64_t n_samples,
                                  int32_t first_frame, int32_t n_frames, double *d_out,
                                  void *stream);

/* Batched form for a recipe slice: n_utts utterances concatenated in d_pcm;
 * utterance u occupies samples [pcm_off[u], pcm_off[u+1]) and emits frames
 * 0 .. last_frame(u) into d_out rows [frame_off[u], frame_off[u+1]).
 * pcm_off/frame_off are HOST arrays of n_utts+1 entries. */
aasr_status aasr_feat_run_batch_dev(aasr_feat *h, const int16_t *d_pcm,
                                    const int64_t *pcm_off,
                                    const int64_t *frame_off, int32_t n_utts,
                                    float *d_out, void *stream);

/* FeatureModule::set_parameters for "normalization" / "lin_transform"
 * (aku/FeatureModules.cc:1094-1117, 1188-1196): params_text is a
 * "{ key value ... }" block as in .spkc files. */
aasr_status aasr_feat_set_parameters(aasr_feat *h, const char *module_name,
                                     const char *params_text);
/* FeatureModule::get_parameters (aku/FeatureModules.cc, per module): the module's adaptation
 * parameters as the same kind of block ("%g" values).  *text is malloc'ed; free it with aasr_free. */
aasr_status aasr_feat_get_parameters(const aasr_feat *h, const char *module_name, char **text,
                                     int64_t *len);
/* FeatureGenerator::module(name) bookkeeping: modules in configuration order
 * (FeatureModule::name / type_str, aku/FeatureModule.hh:47-154); NULL past the end */
int aasr_feat_num_modules(const aasr_feat *h);
const char *aasr_feat_module_name(const aasr_feat *h, int index);
const char *aasr_feat_module_type(const aasr_feat *h, int index);

/* ------------------------------------------------------------------------ */
/* Acoustic model: replaces aku::HmmSet / PDFPool / Mixture scoring          */
/* ------------------------------------------------------------------------ */

/* In-memory construction.  mean/var are [G x dim] row-major doubles as
 * DiagonalGaussian::read stores them (aku/Distributions.cc:1131-1150;
 * var<=0 -> precision 0); mixtures in CSR form: state s owns components
 * mix_off[s] .. mix_off[s+1]-1 with pool indices mix_idx[] (arbitrary, tied
 * pools allowed) and weights mix_w[] (renormalised to sum 1 like
 * Mixture::read, aku/Distributions.cc:2418-2434). */
aasr_status aasr_gmm_create_diag(int32_t dim, int32_t num_gaussians,
                                 const double *mean, const double *var,
                                 int32_t num_states, const int32_t *mix_off,
                                 const int32_t *mix_idx, const double *mix_w,
                                 aasr_gmm **out);
/* Full-covariance pool (FullCovarianceGaussian::read / set_covariance,
 * aku/Distributions.cc:1466-1488, 1559-1586): cov is [G x dim x dim] row-major.
 * Non-SPD covariances become the reference's "invalid" Gaussian (precision and
 * constant 0).  Scored like PDFPool::precompute_likelihoods' exponential-form
 * branch (:2664-2680) but through the Cholesky factor, see DESIGN.md. */
aasr_status aasr_gmm_create_full(int32_t dim, int32_t num_gaussians,
                                 const double *mean, const double *cov,
                                 int32_t num_states, const int32_t *mix_off,
                                 const int32_t *mix_idx, const double *mix_w,
                                 aasr_gmm **out);
/* HmmSet::read_all(base) = read_mc + read_ph + read_gk
 * (aku/HmmSet.cc:351-357); individual paths like phone_probs -g -m -p.
 * ph_path may be NULL (state count = mixture count). */
aasr_status aasr_gmm_create_from_files(const char *gk_path, const char *mc_path,
                                       const char *ph_path, aasr_gmm **out);
/* Binary model cache (new): everything the text parser of
 * aasr_gmm_create_from_files produced, in double precision, with a checksum.
 * A model created from the cache scores bit-identically to one created from
 * the .gk/.mc/.ph files it was written from; the text parse (seconds for a
 * 50 000-Gaussian pool, paid by every per-GPU process of a run) is skipped. */
aasr_status aasr_gmm_write_cache(const aasr_gmm *h, const char *cache_path);
aasr_status aasr_gmm_create_from_cache(const char *cache_path, aasr_gmm **out);
/* The same, for a caller that names the text files too (phone_probs --model-cache):
 * a cache records (size, content hash) of the .gk/.mc/.ph it was written from and
 * is refused (AASR_ERR_INVALID, "stale model cache") when they differ from the
 * files given here -- retraining, or another -b next to the same cache path, then
 * falls back to aasr_gmm_create_from_files instead of scoring with the old model. */
aasr_status aasr_gmm_create_from_cache_checked(const char *cache_path, const char *gk_path,
                                               const char *mc_path, const char *ph_path,
                                               aasr_gmm **out);
void aasr_gmm_destroy(aasr_gmm *h);

/* Model structure for host-side views (aku::Mixture::size / get_base_pdf_index /
 * get_mixture_coefficient, aku/Distributions.hh:795-812; Gaussian::get_mean /
 * get_covariance of a diagonal Gaussian): weights are the normalised ones
 * (Mixture::read -> normalize_weights), index[] / weight[] take
 * aasr_gmm_mixture_size(h, state) values, mean[] / var[] take dim values. */
int32_t aasr_gmm_mixture_size(const aasr_gmm *h, int32_t state);
aasr_status aasr_gmm_mixture_get(const aasr_gmm *h, int32_t state, int32_t *index, double *weight);
aasr_status aasr_gmm_gaussian_get(const aasr_gmm *h, int32_t gaussian, double *mean, double *var);

int aasr_gmm_dim(const aasr_gmm *h);            /* HmmSet::dim()        */
int aasr_gmm_num_states(const aasr_gmm *h);     /* HmmSet::num_states() */
int aasr_gmm_num_gaussians(const aasr_gmm *h);  /* PDFPool::size()      */
/* rows of the component-expanded layout the kernel streams (>= sum n_s) */
int64_t aasr_gmm_expanded_rows(const aasr_gmm *h);

/* Model-side constrained MLLR (ConstrainedMllr::load_transform /
 * AdaptedGaussian, aku/ModelModules.cc:164-232, aku/ModelModules.hh:128-212):
 * pool Gaussian g scores A_t f + b_t instead of f, t = gauss_to_transform[g]
 * (-1 = unadapted), and its likelihood is multiplied by |prod diag A_t| -- the
 * reference's full_matrix_determinant (aku/LinearAlgebra.cc:73-86) returns the
 * product of A's diagonal, kept for parity.  W is [n][dim][dim+1] row-major with
 * column 0 = b_t and columns 1..dim = A_t, the layout of the reference's W
 * matrices.  One transform shared by every Gaussian is applied to the frames
 * (cost of a dim x dim product per frame, like the reference); per-class
 * transforms are folded into per-Gaussian factor rows and scored by the
 * full-covariance kernel.  n_transforms = 0 removes the adaptation
 * (ConstrainedMllr::reset_transform). */
aasr_status aasr_gmm_set_cmllr(aasr_gmm *h, int32_t n_transforms,
                               const int32_t *gauss_to_transform, const double *W);

/* Gaussian clustering: HmmSet::read_clustering / PDFPool::read_clustering
 * (aku/HmmSet.cc:1353-1357, aku/Distributions.cc:3114-3170) and
 * HmmSet::set_clustering_min_evals (aku/HmmSet.cc:1359-1366) -- what
 * phone_probs -C FILE --eval-minc R --eval-ming R sets up
 * (aku/phone_probs.cc:112-117) and PPToolbox::set_clustering
 * (aku/PhoneProbsToolbox.cc:50-53).
 * Once enabled, scoring follows the cluster branch of
 * PDFPool::precompute_likelihoods (aku/Distributions.cc:2684-2722): per frame the
 * cluster centres (unit-weight merges of their members, diagonal) are ranked;
 * members of the best clusters are evaluated exactly until int(min_clusters *
 * clusters) clusters and int(min_gaussians * pool size) Gaussians are done;
 * every other Gaussian takes its centre's likelihood, except where that is 0 in
 * double precision or the Gaussian is in no cluster (PDFPool::compute_likelihood
 * re-evaluates cached values <= 0, aku/Distributions.cc:2636-2644).
 *
 * aasr_gmm_read_clustering reads a .gcl file ("clusters" then "gaussian
 * cluster" pairs).  Like the reference's reader it counts the LAST pair of the
 * file twice (its while(in) loop runs once more on stale operands), which
 * weights that Gaussian double in its centre and in the Gaussian count.
 * aasr_gmm_set_clustering takes the pairs literally (n_clusters = 0 removes the
 * clustering).  Built for diagonal pools (any constrained-MLLR adaptation) and unadapted full-covariance pools, up to
 * 16384 clusters (beyond 4096 every frame takes the slower replay of the reference's priority queue); more than
 * 0.3 * pool size clusters is rejected like the reference does. */
aasr_status aasr_gmm_read_clustering(aasr_gmm *h, const char *gcl_path);
aasr_status aasr_gmm_set_clustering(aasr_gmm *h, int32_t n_clusters, int64_t n_pairs,
                                    const int32_t *gauss_index, const int32_t *cluster_index);
aasr_status aasr_gmm_set_clustering_min_evals(aasr_gmm *h, double min_clusters,
                                              double min_gaussians);
/* PDFPool::number_of_clusters(); 0 without a clustering */
int32_t aasr_gmm_num_clusters(const aasr_gmm *h);

/* Arithmetic used for the frame x Gaussian quadratic forms.
 *  AASR_PREC_F32          f32 matrix-core contraction of the expanded form; models
 *                         whose conditioning would break the 1e-4 budget are
 *                         switched to the centred form automatically
 *  AASR_PREC_F32_CENTRED  always the centred form (x-mu)^2*p on the vector ALU,
 *                         the reference's own arithmetic shape in f32
 *  AASR_PREC_BF16X3       both operands split into three bf16 terms, six
 *                         bf16 matrix-core products per f32 product accumulated
 *                         in f32: f32-class accuracy (same 1e-4 parity bar) at
 *                         ~1.8x the speed of the f32 kernel; diagonal, full-
 *                         covariance and per-class CMLLR models (ill-conditioned
 *                         models still take the centred form).  The environment
 *                         variable AASR_PREC=0 selects AASR_PREC_F32 globally.
 *  AASR_PREC_F16X2        default: both operands as two fp16 terms (22 bits), three
 *                         fp16 matrix-core products per product -- half the matrix
 *                         instructions of BF16X3 at 1.4-1.8x its rounding error, so it
 *                         is used only for models whose conditioning estimate leaves
 *                         that room (same 1e-4 bar, tighter limits: gmm.h
 *                         KAPPA_LIMIT_F16 for diagonal pools, FULL_KAPPA_LIMIT_F16 for the
 *                         factor rows of full-covariance / subspace pools); every other
 *                         model runs as under AASR_PREC_BF16X3.
 *                         aasr_gmm_effective_precision tells which form a model got.
 *  AASR_PREC_F64          the reference's own arithmetic in double, operation by operation (diagonal
 *                         pools; unadapted, under one global CMLLR transform or under per-class transforms, with or
 *                         without clustering): a verification / training-side
 *                         mode, ~1.2 M frames/s at 50 k Gaussians.  Float entry points widen the frames
 *                         and round the scores once; aasr_gmm_score_f64 takes and returns doubles;
 *                         aasr_run_utterance / aasr_run_recipe then run the whole path in double
 *                         (features, scoring, the LNA tail as written) -- AASR_PREC=1 in the
 *                         environment selects it for the command-line tools. */
enum { AASR_PREC_F32 = 0, AASR_PREC_F64 = 1, AASR_PREC_F32_CENTRED = 2, AASR_PREC_BF16X3 = 3, AASR_PREC_F16X2 = 4 };
aasr_status aasr_gmm_set_precision(aasr_gmm *h, int prec);
int aasr_gmm_get_precision(const aasr_gmm *h);
/* the arithmetic the matrix scoring path of this model actually runs under the current setting */
int aasr_gmm_effective_precision(const aasr_gmm *h);
/* Per-state precision routing (new; no aku counterpart -- the reference scores everything in double,
 * aku/Distributions.cc:1040-1062).  States are independent output columns (Mixture::compute_likelihood,
 * aku/Distributions.cc:2078-2086), so under AASR_PREC_F16X2 a diagonal model whose Gaussians do not ALL satisfy the
 * two-term form's conditioning limits is scored in two sections: the states whose Gaussians all qualify with two fp16
 * terms, the others with three bf16 terms (one Gaussian over the limit costs its state the slower arithmetic, not the
 * model).  states_f16x2: how many of the model's states the two-term rows cover under the current setting (0 ... S);
 * states_probe_moved: how many the load-time probe took out of that form (a few hundred frames on the model's own
 * Gaussians, incl. +-6 sigma, scored in f16x2 and in exact f32 when the model is created; a state that differs by more
 * than 5e-5 is scored with three terms).  Either pointer may be null. */
aasr_status aasr_gmm_precision_states(const aasr_gmm *h, int64_t *states_f16x2, int64_t *states_probe_moved);

/* HmmSet::precompute_likelihoods + state_likelihood for a block of frames
 * (aku/HmmSet.cc:484-501, aku/HmmSet.hh:309): frames float32 [F x dim];
 * state_loglik float32 [F x S] = log(max(sum_k w_k exp(ll_k), 1e-50)). */
aasr_status aasr_gmm_score(aasr_gmm *h, const float *frames, int64_t F,
                           float *state_loglik);
/* AASR_PREC_F64 with double frames in and double log state likelihoods out (any precision setting) */
aasr_status aasr_gmm_score_f64(aasr_gmm *h, const double *frames, int64_t F, double *state_loglik);
aasr_status aasr_gmm_score_f64_dev(aasr_gmm *h, const double *d_frames, int64_t F, double *d_state_loglik, void *stream);
aasr_status aasr_gmm_score_dev(aasr_gmm *h, const float *d_frames, int64_t F,
                               float *d_state_loglik, void *stream);

/* PDFPool::precompute_likelihoods (aku/Distributions.cc:2647-2682): the
 * log-likelihood of every pool Gaussian, float32 [F x G]. */
/* The same with a row pitch (floats between consecutive frame rows, >= S) for callers that keep the
 * score matrix on the device: rows padded to a multiple of 32 floats turn every 128-byte output
 * group of the scoring kernel into one whole L2 line (1.1 ms of 32.4 per 10^6 frames x 50 k
 * Gaussians, a quarter less HBM write traffic).  Only the track kernels (f32 and bf16x3) write pitched rows: aasr_gmm_score_pitch_ok() says
 * whether this model / precision does; otherwise pitch must equal the state count. */
int aasr_gmm_score_pitch_ok(const aasr_gmm *h);
aasr_status aasr_gmm_score_dev_pitched(aasr_gmm *h, const float *d_frames, int64_t F,
                                       float *d_state_loglik, int64_t pitch, void *stream);

aasr_status aasr_gmm_gauss_loglik(aasr_gmm *h, const float *frames, int64_t F,
                                  float *gauss_loglik);
aasr_status aasr_gmm_gauss_loglik_dev(aasr_gmm *h, const float *d_frames,
                                      int64_t F, float *d_gauss_loglik,
                                      void *stream);

/* ------------------------------------------------------------------------ */
/* LNA: replaces the frame loop tail of aku/phone_probs.cc:224-262           */
/* ------------------------------------------------------------------------ */

/* state_loglik float32 [F x S] (output of aasr_gmm_score) -> normalised
 * float log-probabilities and LNA bytes.  Emulates the reference's float
 * storage of linear likelihoods (values below FLT_TRUE_MIN flush to 0 ->
 * log(1e-50); denormal quantisation), Z = sum over states (Z==0 or
 * !normalize -> 1), safe_log, then 2-byte big-endian (int)(-1820*lp+.5)
 * (0xFFFF below -36.008) or 4-byte little-endian float.
 * bytes_out: [F x S x lnabytes] (may be NULL); lp_out: [F x S] (may be NULL) */
aasr_status aasr_lna_encode(const float *state_loglik, int64_t F, int32_t S,
                            int normalize, int lnabytes, float *lp_out,
                            uint8_t *bytes_out);
/* device input with a row pitch (see aasr_gmm_score_dev_pitched); outputs are dense */
aasr_status aasr_lna_encode_dev_pitched(const float *d_state_loglik, int64_t in_pitch, int64_t F,
                                        int32_t S, int normalize, int lnabytes, float *d_lp_out,
                                        uint8_t *d_bytes_out, void *stream);
aasr_status aasr_lna_encode_dev(const float *d_state_loglik, int64_t F,
                                int32_t S, int normalize, int lnabytes,
                                float *d_lp_out, uint8_t *d_bytes_out,
                                void *stream);
/* aasr_lna_encode_dev_pitched with the two further arguments of the launch that the engine sets for itself.  d_colmap
 * (device, S entries, may be NULL): state i is read from column d_colmap[i] of an input row, every entry in
 * [0, in_pitch) -- the engine-internal score layout of a routed model; needs S <= 4096 (AASR_ERR_UNSUPPORTED above).
 * wgs_per_cu: the grid of the register-resident kernels (S <= 4096) in workgroups per CU, 1..1024 (AASR_ERR_INVALID
 * outside; every other entry point runs 32).  Neither changes a byte of the output; what the tests of the LNA pass
 * hold it to. */
aasr_status aasr_lna_encode_dev_grid(const float *d_state_loglik, int64_t in_pitch, int64_t F, int32_t S,
                                     int normalize, int lnabytes, const int32_t *d_colmap, int wgs_per_cu,
                                     float *d_lp_out, uint8_t *d_bytes_out, void *stream);
/* aasr_gmm_score_dev_pitched followed by aasr_lna_encode_dev_pitched (bytes only) as one call: afterwards d_scores
 * [F x pitch] and d_bytes [F x S x lnabytes] hold exactly what the two calls leave there, ordered on `stream`.  Where the
 * scoring call is one launch of a track kernel (one-pivot two-term, three-term or f32 layout; no engine parts, clustering,
 * class routing, AASR_PREC_F64 or a pitch the kernel cannot write) the frames are scored in chunks and the LNA pass of a
 * chunk runs on a second stream, owned by the handle, beside the scoring of the next chunk (the frames past the last
 * whole chunk are scored first); `stream` waits for the last LNA pass before the call returns to it.  chunk_frames: frames
 * per chunk, a positive multiple of 512, or 0 for the automatic choice (half a 512-frame block per CU per chunk; fewer
 * than two 512-frame blocks per CU in all: the plain sequence).  Every other
 * case runs the plain sequence on `stream`.  aasr_gmm_score_lna_overlap_active() says whether a call with these arguments
 * takes the two-stream form (1) or the plain sequence (0). */
aasr_status aasr_gmm_score_lna_pitched_dev(aasr_gmm *h, const float *d_frames, int64_t F, float *d_scores, int64_t pitch,
                                           int normalize, int lnabytes, uint8_t *d_bytes, int64_t chunk_frames,
                                           void *stream);
int aasr_gmm_score_lna_overlap_active(const aasr_gmm *h, int64_t F, int64_t pitch, int64_t chunk_frames);
/* Frames straight to LNA codes on the device: aasr_gmm_score_dev followed by
 * aasr_lna_encode_dev, except that the engine may keep the state scores in its
 * own layout in between (rows padded to whole cache lines; a model whose conditioning needs several pivots -- or three
 * terms for part of its states, aasr_gmm_precision_states -- as internal models over disjoint sets of its states, each in
 * its own column range, read back through a column map).  d_scratch takes aasr_gmm_score_scratch_floats(h, F) floats: a
 * property of the MODEL -- it does not change with aasr_gmm_set_precision, clustering or transforms, so a buffer sized
 * once stays valid for the handle's life --, d_bytes_out F * num_states * lnabytes bytes.  What the recipe driver runs
 * per block. */
int64_t aasr_gmm_score_scratch_floats(const aasr_gmm *h, int64_t F);
aasr_status aasr_gmm_score_lna_dev(aasr_gmm *h, const float *d_frames, int64_t F, int normalize, int lnabytes,
                                   float *d_scratch, uint8_t *d_bytes_out, void *stream);

/* 5-byte file header: big-endian uint32 S + 1 byte lnabytes
 * (aku/phone_probs.cc:32-43, 213-214) */
void aasr_lna_header(int32_t num_states, int lnabytes, uint8_t out[5]);

/* Reads an LNA file the way the recogniser's reader does (decoder/src/LnaReaderCircular.cc:
 * header :63-96, frame decoding :166-198): 4-byte little-endian floats, 2-byte big-endian codes
 * (code / -1820.0) or the legacy 1-byte codes (code / -24.0) -- phone_probs never writes the
 * 1-byte form, old acoustic files hold it.  Host only.  A trailing partial frame is dropped, as
 * the reader's fread does.  *log_probs is malloc'ed [*frames x *num_states]; free with aasr_free. */
aasr_status aasr_lna_read_file(const char *path, int32_t *num_states, int32_t *lnabytes, int64_t *frames,
                               float **log_probs);

/* ------------------------------------------------------------------------ */
/* Recipe + whole-path driver: replaces the body of phone_probs main()       */
/* ------------------------------------------------------------------------ */

/* Recipe::read batch selection (aku/Recipe.cc:23-149): returns in
 * first_line/num_lines the contiguous slice of the L non-empty,
 * non-comment recipe lines that batch batch_index (1-based) of num_batches
 * receives (cluster_speakers=false form). */
aasr_status aasr_recipe_batch_range(int32_t num_lines_total, int32_t num_batches,
                                    int32_t batch_index, int32_t *first_line,
                                    int32_t *num_lines);

/* Recipe::read itself (aku/Recipe.cc:23-149), host only: parses recipe text and
 * returns the utterances of one batch as a malloc'ed text table (aasr_free), one
 * line per utterance with the fields audio, lna, speaker, utterance, start-time,
 * end-time separated by 0x1f (times are the float fields of Recipe::Info, printed "%.9g").  Kept from the reference: lines
 * are cleaned of " \t\n" only, fields split on blanks and tabs, `key=value`
 * through str::split (a trailing '=' is dropped), keys persist across lines. */
aasr_status aasr_recipe_read(const char *recipe_text, int32_t num_batches, int32_t batch_index,
                             char **table_out, int64_t *table_len);

/* The same with every field of Recipe::Info (aku/Recipe.hh:40-52) and the cluster_speakers
 * flag of Recipe::read (a batch only ends where the speaker changes, aku/Recipe.cc:86-101):
 * audio, alt-audio, transcript, alignment, hmmnet, den-hmmnet, lna, start-time, end-time,
 * start-line, end-line, speaker, utterance -- 13 fields separated by 0x1f per line. */
aasr_status aasr_recipe_read_all(const char *recipe_text, int32_t num_batches, int32_t batch_index,
                                 int32_t cluster_speakers, char **table_out, int64_t *table_len);

/* start/end frame of an utterance as phone_probs derives them from the recipe's
 * start-time / end-time (aku/phone_probs.cc:199-206): `(int)(time * frame_rate)`
 * with BOTH operands float (Recipe::Info::start_time is a float field,
 * aku/Recipe.hh:48-49; FeatureGenerator::frame_rate() returns float), so the
 * product is rounded to float before truncation; end frame 0 means "to the end"
 * and is returned as INT32_MAX.  Host only. */
void aasr_recipe_frame_limits(float start_time, float end_time, float frame_rate,
                              int32_t *start_frame, int32_t *end_frame);

/* ---------------------------------------------------------------------------
 * User-defined feature module types (the plugin side of aku::FeatureModule,
 * aku/FeatureModule.hh:47-154: a subclass with set_module_config / generate(frame),
 * one more `else if` in FeatureGenerator::load_configuration, aku/FeatureGenerator.cc:145-175).
 * A registered type may appear in any .cfg after the base module.  Its frames are
 * computed by the callback ON THE HOST: when the graph is evaluated, the rows of its
 * sources are copied from the device, `generate` runs once per frame, the result goes
 * back to the device and the modules behind it continue there -- an escape hatch for
 * experiments, not a fast path (the 16 built-in types are kernels).  A built-in
 * name cannot be taken.  The adapter class aku::FeatureModule
 * (aaltoasr_amd/csrc/aku/FeatureModule.hh) wraps this for C++ subclasses.
 *   configure: parse the module's option block ("{\n name value\n ... }\n"), report
 *     the output dimension and how many frames to the left / right of the current
 *     one the module reads from its sources; *instance is handed back to the other
 *     callbacks.  Return 0, or nonzero with a message in err.
 *   generate: sources[k] points at source k's frames frame-left .. frame+right,
 *     row-major [left+right+1][source_dims[k]] doubles (frames outside the file are
 *     the border copies the chain defines); write dim doubles to out. */
typedef struct aasr_host_module {
  int (*configure)(void *user, const char *module_name, const char *options_block, int32_t n_sources,
                   const int32_t *source_dims, int32_t *dim, int32_t *left, int32_t *right, void **instance,
                   char *err, int32_t err_len);
  int (*generate)(void *instance, int32_t frame, const double *const *sources, double *out, char *err,
                  int32_t err_len);
  void (*destroy)(void *instance);
} aasr_host_module;
aasr_status aasr_feat_register_module_type(const char *type_name, const aasr_host_module *vtbl, void *user);

/* ---------------------------------------------------------------------------
 * Speaker / utterance configuration: aku::SpeakerConfig
 * (aku/SpeakerConfig.hh:15-60, aku/SpeakerConfig.cc) -- what phone_probs -S FILE
 * drives (aku/phone_probs.cc:94-95, 191-196).  A .spkc file holds, per speaker
 * and per utterance (and for the "default" of each), parameter blocks for named
 * feature modules ("feature NAME" or just "NAME": normalization, lin_transform,
 * vtln, sr_norm, quanteq take parameters) and for the model module "cmllr"
 * (constrained MLLR matrices w1, w2, ... with unitmode UNIT_NO / UNIT_GAUSSIAN /
 * UNIT_MIX / UNIT_PHONE; the engine maps them onto aasr_gmm_set_cmllr).
 * set_speaker / set_utterance follow the reference step by step, including the
 * read-back of the current speaker's parameters through "%g" before a switch;
 * see aaltoasr_amd/csrc/speaker_config.cc for the list of kept quirks.
 * The handle borrows feat and gmm (gmm may be NULL, or given later with
 * aasr_spkc_set_model -- phone_probs reads the speaker file before the model). */
typedef struct aasr_spkc aasr_spkc;
aasr_status aasr_spkc_create(aasr_feat *feat, aasr_gmm *gmm, aasr_spkc **out);
void aasr_spkc_destroy(aasr_spkc *h);
aasr_status aasr_spkc_set_model(aasr_spkc *h, aasr_gmm *gmm);
/* SpeakerConfig::read_speaker_file */
aasr_status aasr_spkc_read_file(aasr_spkc *h, const char *path);
aasr_status aasr_spkc_read_text(aasr_spkc *h, const char *text);
/* SpeakerConfig::set_speaker / set_utterance; "" (or NULL) selects the default */
aasr_status aasr_spkc_set_speaker(aasr_spkc *h, const char *speaker_id);
aasr_status aasr_spkc_set_utterance(aasr_spkc *h, const char *utterance_id);
/* SpeakerConfig::write_speaker_file (aku/SpeakerConfig.cc:156-236): the speaker file as text, with
 * the current speaker's / utterance's module parameters fetched back first (what the adaptation
 * tools -- vtln, mllr -- write after estimating).  speakers / utterances filter the entries by id
 * ("default" names the default entries); a count < 0 writes all of them.  *text_out is malloc'ed. */
aasr_status aasr_spkc_write_text(aasr_spkc *h, const char *const *speakers, int32_t n_speakers,
                                 const char *const *utterances, int32_t n_utterances, char **text_out,
                                 int64_t *text_len);
/* number of times a module's device parameters were actually rewritten */
int64_t aasr_spkc_num_changes(const aasr_spkc *h);

typedef struct aasr_run_options {
  int32_t lnabytes;        /* 2 or 4          (--lnabytes)          */
  int32_t normalize;       /* 0 = -N / --no-normalization           */
  int32_t num_batches;     /* -B (0/1 = no batching)                */
  int32_t batch_index;     /* -I, 1-based                           */
  int32_t no_overwrite;    /* -n: skip utterances whose LNA exists  */
  int32_t raw_audio;       /* treat inputs as headerless PCM16      */
  int32_t info;            /* -i verbosity                          */
  int32_t afname;          /* -a: name outputs after the audio file */
  const char *out_dir;     /* -o: prefix for LNA paths or NULL      */
  struct aasr_spkc *speakers; /* -S: speaker configuration or NULL   */
  int32_t sort_recipe;     /* --sort-recipe: stable sort of the slice by speaker id
                              (Recipe::sort_infos, aku/Recipe.hh:86-88,115-117) */
} aasr_run_options;

typedef struct aasr_run_stats {
  int64_t utterances;
  int64_t frames;
  double seconds_total;
  double seconds_device;   /* input upload + feature + scoring + LNA kernels (device events) */
  double seconds_copy_out; /* packed rows device -> host; overlaps the next block's kernels */
} aasr_run_stats;

/* phone_probs main loop (aku/phone_probs.cc:145-267) for one recipe slice on
 * the current device: read audio, features, scoring, LNA files. */
aasr_status aasr_run_recipe(aasr_feat *feat, aasr_gmm *gmm,
                            const char *recipe_path,
                            const aasr_run_options *opt, aasr_run_stats *stats);

/* One engine process per GPU: `processes` of them share this host's cores.  The reference scales
 * out the same way -- N independent phone_probs processes on recipe slices (-B n -I k,
 * aku/Recipe.cc:63-115, aku/phone_probs.cc:136-141) -- each single-threaded; here a process runs
 * reader / writer helper threads, and their number is usable_cores / processes (0 = take
 * AASR_LOCAL_RANKS or torchrun's LOCAL_WORLD_SIZE from the environment, else 1). */
aasr_status aasr_set_host_share(int32_t processes);
/* cores this process may use: affinity mask capped by the cgroup CPU quota */
int32_t aasr_host_usable_cores(void);

/* Where the last aasr_run_recipe on this model handle spent its wall time (seconds): what the
 * calling thread waited for, what the two device streams were busy with, and the helper-thread
 * sizing that was in force.  Diagnostics for multi-rank runs; the reference has no counterpart
 * (its loop is serial, aku/phone_probs.cc:145-267). */
typedef struct aasr_recipe_timing {
  double seconds_total;
  double wait_reader;       /* calling thread idle: next utterance not read yet           */
  double wait_result_slot;  /* ... idle: both pinned result slots still being written out */
  double enqueue;           /* ... enqueueing a block (incl. pageable uploads)            */
  double wait_copies;       /* ... waiting for a block's device -> host copy              */
  double device;            /* compute stream busy (upload + features + scoring + LNA)    */
  double copy_out;          /* copy stream busy (packed rows device -> host)              */
  int32_t writer_threads;
  int32_t usable_cores;
  int32_t host_share;
} aasr_recipe_timing;
aasr_status aasr_recipe_last_timing(const aasr_gmm *gmm, aasr_recipe_timing *out);

/* PPToolbox::generate_from_file_to_fd equivalent for one utterance
 * (aku/PhoneProbsToolbox.cc:135-208: lnabytes 2, normalised): returns a
 * malloc'ed LNA image (header + frames) the caller frees with aasr_free. */
aasr_status aasr_run_utterance(aasr_feat *feat, aasr_gmm *gmm,
                               const int16_t *pcm, int64_t n_samples,
                               int32_t start_frame, int32_t end_frame,
                               int normalize, int lnabytes, uint8_t **lna_out,
                               int64_t *lna_len, int64_t *frames_out);
void aasr_free(void *p);

/* Audio input of the audiofile module, host only (no device needed).  Replaces
 * AudioReader::open + check_audio_parameters + read_from_file
 * (aku/AudioReader.cc:86-110, 145-156, 170-213) and AudioFileModule::set_fname's
 * sample-rate check (aku/FeatureModules.cc:244-262): RIFF/WAVE, AU, AIFF/AIFF-C
 * and NIST SPHERE files holding integer PCM or G.711, converted to 16-bit the
 * way sf_read_short() does; anything else is read as headerless PCM16 in the
 * module's byte order -- the reference's fallback.  `feat` supplies the
 * module's `sample_rate`, `raw` and `endian` options (NULL: no rate check,
 * container detection on, little endian).  *pcm is malloc'ed; free it with
 * aasr_free. */
aasr_status aasr_audio_read(const aasr_feat *feat, const char *path, int16_t **pcm,
                            int64_t *n_samples, int32_t *sample_rate);

/* The same decoding for input already in memory -- what FeatureGenerator::open(FILE*, ...) /
 * open_fd (aku/FeatureGenerator.cc:54-84) and PPToolbox::generate_to_fd (aku/PhoneProbsToolbox.cc:
 * 55-82) read from a descriptor.  For graphs that start with a `pre` module the data is a feature
 * file and *pcm receives the engine's input units for it (see aasr_feat_input_is_features). */
aasr_status aasr_audio_decode(const aasr_feat *feat, const void *data, int64_t n_bytes, int16_t **pcm,
                              int64_t *n_samples, int32_t *sample_rate);

/* ---------------------------------------------------------------------------
 * Forced alignment: aku/align.cc with aku/Viterbi.cc and aku/Lattice.cc, the Viterbi search on the
 * device (csrc/align_viterbi.hip, one wave per utterance, many utterances per launch).
 *
 * Topology: the HMMs of a legacy PHONE .ph file with their transitions (aku/HmmSet.cc:183-329; the
 * same reader as the aku::HmmSet adapter).  States are tied by pdf index; a transition to the
 * dummy final state is stored as the offset that leaves the HMM (+1 past its last state).  The
 * handle is separate from aasr_gmm: scoring and the model cache do not see it. */
typedef struct aasr_topo aasr_topo;
aasr_status aasr_topo_create_from_ph(const char *ph_path, aasr_topo **out);
void aasr_topo_destroy(aasr_topo *h);
int32_t aasr_topo_num_hmms(const aasr_topo *h);
/* HmmSet::hmm_index: -1 for an unknown label */
int32_t aasr_topo_hmm_index(const aasr_topo *h, const char *label);
const char *aasr_topo_hmm_label(const aasr_topo *h, int32_t hmm);
int32_t aasr_topo_hmm_num_states(const aasr_topo *h, int32_t hmm);
/* the HMM's state (= pdf) indices, hmm_num_states entries */
aasr_status aasr_topo_hmm_states(const aasr_topo *h, int32_t hmm, int32_t *states);
/* number of states the file mentions (largest pdf index + 1) */
int32_t aasr_topo_num_states(const aasr_topo *h);
int32_t aasr_topo_state_num_transitions(const aasr_topo *h, int32_t state);
/* the state's transitions in file order: target offset (relative position) and probability */
aasr_status aasr_topo_state_transitions(const aasr_topo *h, int32_t state, int32_t *target_offset, double *prob);
int32_t aasr_topo_max_offset(const aasr_topo *h);
/* every state index below aasr_gmm_num_states and every target offset <= 255 (the search's
 * back-pointer encoding); AASR_ERR_INVALID naming the HMM otherwise */
aasr_status aasr_topo_validate(const aasr_topo *h, const aasr_gmm *gmm);
/* the same checks against a state count (host only: what aasr_topo_validate runs with
 * aasr_gmm_num_states(gmm)) */
aasr_status aasr_topo_check_states(const aasr_topo *h, int32_t num_states);

typedef struct aasr_align_options {
  int32_t swins;         /* --swins: window size in frames and positions (1000)        */
  double beam;           /* --beam: log-probability beam (100)                         */
  int32_t sbeam;         /* --sbeam: state beam (100)                                  */
  double maxbeam;        /* --maxbeam: retries double the beams up to this (1600)      */
  float overlap;         /* --overlap: window overlap (0.4); a window commits          */
                         /* (int)(swins * (1 - overlap)) frames, which must be         */
                         /* 1 .. swins - 1: overlap <= 0, >= 1 or not finite is invalid */
  int32_t no_force_end;  /* --no-force-end                                             */
  int32_t phoseg;        /* --phoseg: phone segmentation instead of states             */
  int32_t info;          /* -i                                                         */
  int32_t num_batches;   /* -B                                                         */
  int32_t batch_index;   /* -I                                                         */
  struct aasr_spkc *speakers; /* -S: speaker configuration or NULL                     */
} aasr_align_options;
void aasr_align_default_options(aasr_align_options *opt);

/* A transcript as aku/PhnReader.cc:294-400 reads it for align: "label [comment]" lines or
 * "start end label[.state] [comment]" lines (sample numbers at 16 kHz), empty lines skipped, the
 * frame limits of a recipe line applied (first_frame / last_frame as PhnReader::set_frame_limits,
 * both 0: none).  Per line, *line_hmms receives the HMM index the line adds, or -1 for a line whose
 * state field is > 0 (it adds none).  An unknown label is AASR_ERR_INVALID naming label and file.
 * *line_hmms is malloc'ed (aasr_free). */
aasr_status aasr_align_read_transcript(const aasr_topo *topo, const char *path, float frame_rate,
                                       int32_t first_frame, int32_t last_frame, int32_t **line_hmms,
                                       int32_t *n_lines);
/* One line of an alignment file (align.cc:print_line): "start*m end*m label comment\n" with
 * m = (int)(16000 / frame_rate); nothing for start < 0.  Returns the length written (< cap). */
int32_t aasr_align_format_line(float frame_rate, int32_t start, int32_t end, const char *label,
                               const char *comment, char *buf, int32_t cap);

/* Batched search.  A batch holds n_utt utterances: their transcripts (lines [line_off[u],
 * line_off[u+1]) of line_hmms), first frame, end frame ((int)(end_time * frame_rate), 0: to the end of the
 * audio) and eof frame (aasr_feat_eof_frame).  It carries each utterance's lattice on the device
 * between calls. */
typedef struct aasr_align_batch aasr_align_batch;
aasr_status aasr_align_batch_create(const aasr_topo *topo, const aasr_align_options *opt, int32_t n_utt,
                                    const int32_t *line_off, const int32_t *line_hmms,
                                    const int32_t *start_frame, const int32_t *end_frame,
                                    const int32_t *eof_frame, aasr_align_batch **out);
void aasr_align_batch_destroy(aasr_align_batch *b);
/* score rows each utterance reads: frames start_frame .. min(eof, end) - 1, at least one */
int32_t aasr_align_batch_rows(const aasr_align_batch *b, int32_t u);
/* device bytes the batch holds (lattice rings, transcripts, outputs) */
int64_t aasr_align_batch_device_bytes(const aasr_align_batch *b);
/* Enqueues `windows` window steps (>= 1) of every active utterance on `stream`, no host wait.
 * d_state_loglik: state log-likelihood rows on the device (float, or double when f64 -- the
 * AASR_PREC_F64 rows), `pitch` elements apart; row0[u] (host) is the row of utterance u's first
 * frame.  gmm is the model the rows were scored with (its state count bounds the topology). */
aasr_status aasr_align_batch_dev(const aasr_gmm *gmm, aasr_align_batch *b, const void *d_state_loglik,
                                 int64_t pitch, int32_t f64, const int64_t *row0, int32_t windows,
                                 void *stream);
/* Waits for `stream` and fetches the per-utterance results; *n_active: utterances still running. */
aasr_status aasr_align_batch_sync(aasr_align_batch *b, void *stream, int32_t *n_active);
enum { AASR_ALIGN_ACTIVE = 0, AASR_ALIGN_OK = 1, AASR_ALIGN_GAVE_UP = 2, AASR_ALIGN_ERROR = 3 };
/* Results after a sync: the committed absolute transcription position of each frame from the first
 * (n_committed of them; positions may be NULL), the log-likelihood (Viterbi::best_path_log_prob),
 * the status, how many times the forced end was missed (each miss doubled beam and state beam;
 * status OK with n_fail > 0: retried, GAVE_UP: beyond maxbeam). */
aasr_status aasr_align_batch_result(const aasr_align_batch *b, int32_t u, int32_t *positions,
                                    int32_t *n_committed, double *loglik, int32_t *status,
                                    int32_t *n_fail);

/* align main loop (aku/align.cc:171-346) over one recipe slice: audio, transcripts, features and
 * scores per utterance (speaker configuration applied per utterance), the search for many
 * utterances at once on the device, .phn files and the -i diagnostics on stderr. */
aasr_status aasr_run_align_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo,
                                  const char *recipe_path, const aasr_align_options *opt,
                                  aasr_run_stats *stats);

/* ---------------------------------------------------------------------------
 * Maximum-likelihood statistics: aku/stats.cc with --ml over state-segmented .phn files (PhnReader),
 * accumulated on the device (csrc/stats_accum.hip) and dumped as HmmSet::dump_statistics writes
 * them (.gks, .mcs, .phs) with the .lls summary, for the reference's estimate / combine_stats.
 * Diagonal pools without model-side transforms only; -H (hmmnets) and MMI / MPE are not built.  With
 * full statistics (aasr_stats_create_full, the tool's --full-stats) the second moment of every Gaussian is
 * the whole matrix sum gamma x x^T (csrc/stats_full_accum.hip) and the dumps are mode 3
 * (PDF_ML_STATS | PDF_ML_FULL_STATS): what estimate --mllt reads, what the reference's stats --mllt writes.
 *
 * Segmentation: PhnReader::next_frame (aku/PhnReader.cc:138-292) as stats configures it -- the emission
 * pdf of every frame from the first line's start on, and with `transitions` the global index of the
 * transition taken (HmmSet::read_ph order, -1 on the last frame).  first_frame / last_frame: the recipe's
 * frame limits (both 0: none); the frames stop at eof_frame (aasr_feat_eof_frame; < 0: no limit).
 * *n_frames = -1 when the file holds no line ("Could not initialize the utterance segmentation").
 * *pdf and *transition are malloc'ed (aasr_free).  Host only. */
aasr_status aasr_stats_read_segmentation(const aasr_topo *topo, const char *path, float frame_rate,
                                         int32_t first_frame, int32_t last_frame, int32_t eof_frame,
                                         int32_t transitions, int32_t *start_frame, int32_t **pdf,
                                         int32_t **transition, int32_t *n_frames);

/* Dump writers over plain host arrays (HmmSet.cc:546-625, Distributions.cc:157-172, 305-315,
 * 2192-2208).  A Gaussian is written as accumulated when feacount > 0, a mixture when count (its
 * frames with a positive total likelihood) > 0, a transition when its count > 0.  sum_x / sum_xx are
 * [pool_size x dim] and go out as float; mode is the statistics mode (1: ML).  Host only. */
aasr_status aasr_stats_write_gks(const char *path, int32_t pool_size, int32_t dim, int32_t mode,
                                 const int64_t *feacount, const double *gamma, const double *aux_gamma,
                                 const double *sum_x, const double *sum_xx);
/* The mode-3 .gks (FullStatisticsAccumulator::dump_statistics, Distributions.cc:42-60): per accumulated Gaussian the
 * means as floats, then sum_xx_packed [pool_size x dim (dim + 1) / 2], the lower triangle row by row (j <= i), as
 * floats.  Host only. */
aasr_status aasr_stats_write_gks_full(const char *path, int32_t pool_size, int32_t dim, const int64_t *feacount,
                                      const double *gamma, const double *aux_gamma, const double *sum_x,
                                      const double *sum_xx_packed);
aasr_status aasr_stats_write_mcs(const char *path, int32_t num_pdfs, int32_t mode, const int32_t *mix_off,
                                 const int32_t *mix_idx, const int64_t *count, const double *gamma,
                                 const double *aux_gamma, const double *mixture_ll);
aasr_status aasr_stats_write_phs(const char *path, int32_t num_transitions, const int32_t *source,
                                 const int32_t *target_offset, const double *count);
aasr_status aasr_stats_write_lls(const char *path, double loglik, int64_t frames);

/* The accumulator of one model and topology, on the device.  Sums of every mixture component
 * (gamma, aux gamma, sum gamma x, sum gamma x^2), per mixture its frames and mixture_ll, per transition
 * its count (host).  Deterministic: no atomics, fixed summation order. */
typedef struct aasr_stats aasr_stats;
aasr_status aasr_stats_create(aasr_gmm *gmm, const aasr_topo *topo, aasr_stats **out);
/* The same handle with full statistics: every aasr_stats_accumulate_dev call also adds, on the same stream, per pool
 * Gaussian sum gamma xi xi^T with xi = [1, x] over the frames of every mixture that holds it (on the FP64 matrix
 * pipe; per Gaussian: pdfs ascending, work items in order, components in record order; no atomics).  Everything else
 * behaves, byte for byte, as on a handle of aasr_stats_create.  At most 127 dimensions (AASR_ERR_UNSUPPORTED above,
 * before anything is allocated); the accumulator takes 12 KiB per Gaussian at 39 dimensions, 72 KiB at 127. */
aasr_status aasr_stats_create_full(aasr_gmm *gmm, const aasr_topo *topo, aasr_stats **out);
/* the statistics mode of the handle's dumps: 1, or 3 with full statistics */
int32_t aasr_stats_mode(const aasr_stats *h);
void aasr_stats_destroy(aasr_stats *h);
/* Adds n_frames double frame rows (device, [n_frames x dim]) whose pdfs are pdf[] (host; -1: skip)
 * on `stream`, no host wait.  d_frame_ll (device, n_frames doubles, or NULL) receives every frame's
 * safe_log(state likelihood).  Calls on one handle go to one stream. */
aasr_status aasr_stats_accumulate_dev(aasr_stats *h, const double *d_frames, int64_t n_frames,
                                      const int32_t *pdf, double *d_frame_ll, void *stream);
/* Adds weighted entries: cnt (host, states + 1; cnt[s] the first entry of pdf s) describes d_rows / d_weights (device,
 * cnt[states] elements): entry e of pdf s is frame row d_rows[e] of d_frames with Mixture::accumulate's gamma
 * d_weights[e] (aku/Distributions.cc:2134-2161): posteriors gamma * weight * lik / total, mixture_ll += gamma *
 * safe_log(total) also where total is 0, the frame count and feacount one up per entry with total > 0, aux gamma fabs.
 * A frame may appear under several pdfs.  With every weight 1.0 and the row list of aasr_stats_accumulate_dev the sums
 * are that call's, byte for byte; the two may be mixed on one handle.  On `stream`, no host wait
 * (csrc/stats_weighted.hip).  A handle of aasr_stats_create_full refuses it (AASR_ERR_UNSUPPORTED, nothing queued). */
aasr_status aasr_stats_accumulate_weighted_dev(aasr_stats *h, const double *d_frames, int64_t n_frames, const int64_t *cnt,
                                               const int32_t *d_rows, const double *d_weights, void *stream);
/* counts the transitions transition[0..n) (-1: none) */
aasr_status aasr_stats_add_transitions(aasr_stats *h, const int32_t *transition, int64_t n);
/* sums the Gaussians that several mixtures share and fetches everything to the host (waits) */
aasr_status aasr_stats_fetch(aasr_stats *h, void *stream);
/* after a fetch: per pool Gaussian (sum_x / sum_xx [pool x dim]); per pdf its frame count and
 * mixture_ll and per mixture component (aasr_gmm record order) its gamma; any pointer may be NULL */
aasr_status aasr_stats_gaussians(const aasr_stats *h, int64_t *feacount, double *gamma, double *aux_gamma,
                                 double *sum_x, double *sum_xx);
aasr_status aasr_stats_mixtures(const aasr_stats *h, int64_t *count, double *gamma, double *mixture_ll);
/* after a fetch, full handles only (AASR_ERR_INVALID on others): sum_xx [pool x dim (dim + 1) / 2], the packed lower
 * triangles of sum gamma x x^T, row-major with j <= i (the layout of aasr_estimate_get_statistics in mode 3 and of
 * aasr_mllt_create); zeros for a Gaussian without frames */
aasr_status aasr_stats_full_moments(const aasr_stats *h, double *sum_xx);
int32_t aasr_stats_num_transitions(const aasr_stats *h);
aasr_status aasr_stats_transitions(const aasr_stats *h, int32_t *source, int32_t *target_offset, double *count);
/* Diagnostic, read-only: the launch shape of the last aasr_stats_accumulate_dev / _weighted_dev call that reached the
 * accumulation kernel -- out[0] the kernel's dimension instance, out[1] frames per sub-block (256, 192,
 * 128 or 64), out[2] 1 when the mixture records were staged in LDS, out[3] the model's largest mixture,
 * out[4] work items launched.  Five zeros before the first such call. */
void aasr_debug_stats_shape(const aasr_stats *h, int32_t *out);
/* Diagnostic, read-only: the full pass of the last aasr_stats_accumulate_dev call that reached it -- out[0] PB (the
 * blocks of 16 that dim + 1 is padded to), out[1] work items, out[2] launches, out[3] units (item x component).
 * Four zeros before the first such call and on a handle without full statistics. */
void aasr_debug_stats_full_shape(const aasr_stats *h, int32_t *out);
/* Diagnostic: the bound on a launch's slab memory in the full pass (default 64 MiB; one work item at least).  The
 * result's bytes do not depend on it.  Full handles only. */
aasr_status aasr_debug_stats_set_slab_bytes(aasr_stats *h, int64_t bytes);
/* after a fetch: base.phs, base.mcs, base.gks (mode 3 on a full handle) */
aasr_status aasr_stats_write(const aasr_stats *h, const char *base);

typedef struct aasr_stats_options {
  int32_t transitions;  /* -t: transition statistics                       */
  int32_t ophn;         /* -O: read the recipe's alignment= files            */
  int32_t no_train;     /* -n: only the .lls summary                         */
  int32_t uttadap;      /* -U: utterance adaptation                          */
  int32_t info;         /* -i                                                */
  int32_t num_batches;  /* -B                                                */
  int32_t batch_index;  /* -I                                                */
  struct aasr_spkc *speakers; /* -S: speaker configuration or NULL          */
  const char *out;      /* -o: base name of the output files                 */
  int32_t full_stats;   /* --full-stats: full second moments, mode-3 dumps   */
} aasr_stats_options;
void aasr_stats_default_options(aasr_stats_options *opt);
/* What Baum-Welch over HMM networks adds (aasr_run_stats_networks_recipe).  A struct of its own: aasr_stats_options ends
 * with full_stats for its callers. */
typedef struct aasr_stats_network_options {
  int32_t viterbi;        /* -M vit: the best path instead of Baum-Welch          */
  int32_t ac_scale_given; /* 1: -A was on the command line                        */
  double fw_beam;         /* -F: 0 keeps the default 15 (set_pruning_thresholds)  */
  double bw_beam;         /* -W: 0 keeps the default 200                          */
  double ac_scale;        /* -A                                                   */
  int32_t alignment;      /* -a: write the best path's state alignment to each line's alignment= file (-M vit only) */
} aasr_stats_network_options;
void aasr_stats_network_default_options(aasr_stats_network_options *opt);

/* stats main loop (aku/stats.cc:540-795, --ml with .phn segmentations) over one recipe slice: audio,
 * speaker configuration, features on the device and segmentations per utterance, the accumulation
 * for many utterances per launch, the dumps and out.lls, the -i messages on stderr. */
aasr_status aasr_run_stats_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo,
                                  const char *recipe_path, const aasr_stats_options *opt,
                                  aasr_run_stats *stats);
/* The same loop with Baum-Welch over the recipe's hmmnet= networks in place of the .phn files (the reference's
 * stats -H): per group of utterances the state rows of the model's scoring entry in the model's precision mode, the
 * forward-backward pass (aasr_fb_batch_*; retries as simple_train, aku/stats.cc:79-102: 2x ... 5x the backward beam, the
 * reference's messages, a given-up utterance adds nothing), the occupancies as weighted entries into the accumulation
 * (aasr_fb_batch_entries_dev, aasr_stats_accumulate_weighted_dev), with opt->transitions the pass's transition
 * occupancies (summed over frames, not divided by the frame's probability sum), and out.lls with the sum of the forward
 * totals and the frames of the utterances that ran.  A line without hmmnet= is the reference's error; a frame whose
 * probabilities sum to less than 0.01 (where the reference exits) is AASR_ERR_INVALID.  Refused (AASR_ERR_UNSUPPORTED):
 * opt->full_stats, opt->ophn.  net NULL: the defaults.
 * With net->alignment (and net->viterbi; AASR_ERR_UNSUPPORTED under Baum-Welch, where no single arc belongs to a frame) every
 * utterance's alignment= file is written as aku/stats.cc writes it (:116-131, 179-188): a frame's label is its arc's label
 * (transition index and the ";..." part, '#' end marks dropped), "fields[2].fields[1]" where that splits at ';' into three
 * or more fields (HmmNetBaumWelch.cc:763-768); runs of one label make a line "start end label", in samples at 16 kHz
 * ((int)(16000 / frame_rate) per frame), frames counted from the line's start time; the last line ends one frame past the
 * range, the reference's own "+1".  A file that cannot be opened is the reference's message on stderr and the utterance
 * runs without it; a given-up utterance leaves its file empty.  opt->no_train still writes the alignments. */
aasr_status aasr_run_stats_networks_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo,
                                           const char *recipe_path, const aasr_stats_options *opt,
                                           const aasr_stats_network_options *net, aasr_run_stats *stats);

/* ---------------------------------------------------------------------------
 * The log-likelihood of a state segmentation, per frame: what aku/vtln.cc:99-114 asks of the model for every frame,
 * safe_log(Mixture::compute_likelihood(frame)) of the one pdf the segmentation gives it -- the d_frame_ll of
 * aasr_stats_accumulate_dev, byte for byte, from a kernel of its own (csrc/seg_loglik.hip) that sums nothing: any
 * dimension and any mixture size.  Refused at create with AASR_ERR_UNSUPPORTED, before the device is asked for
 * anything: full-covariance Gaussians, subspace Gaussians, model-side transforms.  Deterministic: no atomics. */
typedef struct aasr_segll aasr_segll;
aasr_status aasr_segll_create(aasr_gmm *gmm, aasr_segll **out);
void aasr_segll_destroy(aasr_segll *h);
/* n_frames double frame rows (device, [n_frames x dim]) whose pdfs are pdf[] (host) -> d_frame_ll (device, n_frames
 * doubles) on `stream`, no host wait.  A frame with pdf -1 (any negative pdf) is skipped: its entry of d_frame_ll is
 * not written.  A pdf >= the number of states is AASR_ERR_INVALID and nothing is queued.  Calls on one handle go to
 * one stream. */
aasr_status aasr_segll_score_dev(aasr_segll *h, const double *d_frames, int64_t n_frames,
                                 const int32_t *pdf, double *d_frame_ll, void *stream);
/* Diagnostic, read-only: the last aasr_segll_score_dev call that launched the kernel -- out[0] work items (one pdf,
 * at most 256 rows each), out[1] rows per LDS sub-block (no more than the largest item has), out[2] LDS bytes of a
 * workgroup (at most 65536), out[3] doubles between two rows in LDS, out[4] rows of the largest item.  Five zeros
 * before the first such call. */
void aasr_debug_segll_shape(const aasr_segll *h, int32_t *out);

/* PhnReader::next_frame (aku/PhnReader.cc:138-292) with the reader's two modes: aasr_stats_read_segmentation with
 * `flags`, a sum of
 *   AASR_PHN_STATE_NUM_LABELS  --snl: the first field after the times is the state's index (atoi; no HMM label is
 *                              looked up).  With `transitions` the call is refused (AASR_ERR_UNSUPPORTED).
 *   AASR_PHN_RELATIVE_SAMPLES  --rsamp: the file's times count from first_frame (start and end are shifted by it) and
 *                              no line is skipped for first_frame.
 * flags = 0 is aasr_stats_read_segmentation.  Host only. */
#define AASR_PHN_STATE_NUM_LABELS 1
#define AASR_PHN_RELATIVE_SAMPLES 2
aasr_status aasr_phn_read_segmentation(const aasr_topo *topo, const char *path, float frame_rate,
                                       int32_t first_frame, int32_t last_frame, int32_t eof_frame, int32_t flags,
                                       int32_t transitions, int32_t *start_frame, int32_t **pdf,
                                       int32_t **transition, int32_t *n_frames);

/* ---------------------------------------------------------------------------
 * VTLN warp-factor estimation: aku/vtln.cc over state-segmented .phn files.  Per speaker a grid of warp factors
 * around a centre (1, or with `relative` the speaker's current factor); per grid point the utterances' features under
 * that factor and the log-likelihood of their segmentations (aasr_segll), summed per speaker in recipe order and
 * frame order; the best factor of every speaker is set on the module and the speaker configuration. */
typedef struct aasr_vtln_options {
  int32_t ophn;            /* -O: read the recipe's alignment= files              */
  int32_t snl;             /* --snl: state-number labels                          */
  int32_t rsamp;           /* --rsamp: sample numbers relative to the start time  */
  int32_t info;            /* -i                                                  */
  int32_t num_batches;     /* -B                                                  */
  int32_t batch_index;     /* -I                                                  */
  int32_t grid_size;       /* --grid-size (21)                                    */
  int32_t grid_size_given; /* 1: --grid-size was on the command line              */
  float grid_rad;          /* --grid-rad (0.1)                                    */
  int32_t grid_rad_given;  /* 1: --grid-rad was on the command line               */
  int32_t relative;        /* --relative                                          */
  const char *module;      /* -v: the vtln module                                 */
  struct aasr_spkc *speakers; /* -S: the speaker configuration (required)         */
  const char *out;         /* -o: the speaker file to write, or NULL              */
  const char *savesum;     /* -s: the summary file to write, or NULL              */
} aasr_vtln_options;
void aasr_vtln_default_options(aasr_vtln_options *opt);
/* The grid of aku/vtln.cc:214-225 in float: grid_start (negated, as the loop uses it), grid_step, grid_size.  Host only. */
void aasr_vtln_grid(const aasr_vtln_options *opt, float *grid_start, float *grid_step, int32_t *grid_size);
/* save_vtln_stats (aku/vtln.cc:118-129): per speaker, in the order of the ids' bytes, "[id]", a "%.3f: %.3f" line per
 * warp factor and an empty line.  counts[i] factors of speaker i follow each other in warps / logliks.  *text is
 * malloc'ed (aasr_free).  Host only. */
aasr_status aasr_vtln_summary_text(const char *const *speakers, int32_t n_speakers, const int32_t *counts,
                                   const float *warps, const double *logliks, char **text, int64_t *len);
/* Diagnostic: the bound on a group's frames in aasr_run_vtln_recipe (default 2^20; a group holds one utterance at
 * least).  The files written do not depend on it.  <= 0: the default again. */
void aasr_debug_vtln_set_group_frames(int64_t frames);
/* vtln main loop (aku/vtln.cc:234-286) over one recipe slice (read with cluster_speakers). */
aasr_status aasr_run_vtln_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo,
                                 const char *recipe_path, const aasr_vtln_options *opt,
                                 aasr_run_stats *stats);

/* ---------------------------------------------------------------------------
 * HMM networks and the forward-backward pass over them (aku/HmmNetBaumWelch.cc).
 *
 * aasr_hmmnet_read: HmmNetBaumWelch::read_fst (aku/HmmNetBaumWelch.cc:65-163) with check_network_structure (:536-617)
 * and the topological-order check of :165-289, all with the reference's messages (aasr_last_error).  The text FST has
 * "I node", "F node" and "T src dst [in [out [score]]]" lines; "," is the epsilon string, a "#..." input label an
 * epsilon arc, any other label starts with the global transition index (HmmSet::read_ph order, the numbering of
 * aasr_stats_read_segmentation) and may go on with ";..." higher-level labels, which are kept as text only: the
 * logical-arc hierarchy is not built.  Host only, works without a device. */
typedef struct aasr_hmmnet aasr_hmmnet;
aasr_status aasr_hmmnet_read(const aasr_topo *topo, const char *path, aasr_hmmnet **out);
void aasr_hmmnet_destroy(aasr_hmmnet *net);
/* counts[AASR_HMMNET_NUM_COUNTS]: nodes, emitting arcs, epsilon arcs, backward epsilon levels, forward epsilon levels,
 * distinct pdfs, distinct transition indices, initial node, final node */
#define AASR_HMMNET_NUM_COUNTS 9
aasr_status aasr_hmmnet_counts(const aasr_hmmnet *net, int32_t *counts);
/* The reader's flat arrays (csrc/hmmnet.h).  int32 arrays 0..22: em_begin, em_src, em_tgt, em_pdf, em_tr, em_self,
 * in_begin, in_arcs, pdfs, pdf_begin, pdf_arcs, trs, tr_begin, tr_arcs, eo_begin, ep_src, ep_tgt, ei_begin, ei_arcs,
 * bl_begin, bl_nodes, fl_begin, fl_nodes; double arrays 100..102: em_logp, em_static, ep_score.  *count receives the
 * length; the array is copied when out is given and capacity (elements) suffices. */
aasr_status aasr_hmmnet_array(const aasr_hmmnet *net, int32_t which, void *out, int64_t capacity, int64_t *count);
/* the ";..." part of emitting arc `arc`'s label ("" without one); NULL out of range */
const char *aasr_hmmnet_arc_label(const aasr_hmmnet *net, int32_t arc);

/* The batched pass: fill_backward_probabilities (aku/HmmNetBaumWelch.cc:817-1020) with
 * backward_propagate_epsilon_arcs (:1023-1075), then create_segmented_lattice (:1078-1419), arc scores as
 * get_arc_score (:1917-1942) with static scores and transition probabilities on, in dense form on the device
 * (csrc/hmmnet_fb.hip): one workgroup per utterance, double arithmetic, no atomics, fixed summation orders. */
#define AASR_FB_BAUM_WELCH 0
#define AASR_FB_VITERBI 1
#define AASR_FB_OK 1              /* both passes ran                                                    */
#define AASR_FB_FAILED_BACKWARD 2 /* the backward pass did not reach the initial node (widen the beam) */
#define AASR_FB_FAILED_FORWARD 3  /* no token survived the forward pass                                 */
typedef struct aasr_fb_options {
  double fw_beam;        /* -F (15), set_pruning_thresholds (:526-532)                                        */
  double bw_beam;        /* -W (200)                                                                          */
  double ac_scale;       /* -A (1), set_acoustic_scaling                                                      */
  int32_t mode;          /* AASR_FB_BAUM_WELCH, or AASR_FB_VITERBI (-V)                                       */
  int32_t max_attempts;  /* attempt k runs with backward beam k x bw_beam (aku/logl.cc:183-199: 5)            */
  int32_t want_pdf_occ;  /* keep, per frame, the occupancy of every pdf of the network's pdf list             */
  int32_t want_tr_occ;   /* keep, per transition index of the network, the occupancy summed over the frames   */
  int32_t force_global;  /* node vectors in global memory whatever the networks' size (csrc/hmmnet_fb.h)      */
  int32_t device_occ;    /* with want_pdf_occ: the occupancies stay on the device for aasr_fb_batch_entries_dev --
                            aasr_fb_batch_sync copies none and aasr_fb_batch_result refuses pdf_occ; 0: as before  */
  int32_t want_path;     /* AASR_FB_VITERBI only (AASR_ERR_UNSUPPORTED otherwise): keep the emitting arc taken at
                            every frame for aasr_fb_batch_path; 0: every other output keeps its bytes              */
} aasr_fb_options;
void aasr_fb_default_options(aasr_fb_options *opt);
typedef struct aasr_fb_batch aasr_fb_batch;
/* nets[u] (alive as long as the batch) and the number of frames of utterance u (the frame range last - first of
 * HmmNetBaumWelch::set_frame_limits, at least 1) */
aasr_status aasr_fb_batch_create(const aasr_fb_options *opt, int32_t n_utt, const aasr_hmmnet *const *nets,
                                 const int32_t *n_frames, aasr_fb_batch **out);
void aasr_fb_batch_destroy(aasr_fb_batch *b);
int64_t aasr_fb_batch_device_bytes(const aasr_fb_batch *b);
/* State log-likelihood rows already on the device, as aasr_align_batch_dev takes them: float rows, or double rows when
 * f64, `pitch` elements apart, n_rows of them; row0[u] is the row of utterance u's first frame.  attempt 1 runs every
 * utterance with the options' backward beam; attempt k > 1 is a new launch over the utterances that the last
 * aasr_fb_batch_sync found with AASR_FB_FAILED_BACKWARD only, with backward beam k x bw_beam and the forward beam
 * unchanged (aku/logl.cc:183-199).  Returns when the launch has been queued and its tables copied. */
aasr_status aasr_fb_batch_dev(aasr_fb_batch *b, const void *d_state_loglik, int64_t pitch, int64_t n_rows, int32_t f64,
                              const int64_t *row0, int32_t attempt, void *stream);
/* waits for the stream and fetches the results; *n_failed_backward: utterances a further attempt would run */
aasr_status aasr_fb_batch_sync(aasr_fb_batch *b, void *stream, int32_t *n_failed_backward);
/* After a sync.  backward_total: the initial node's score after the first frame (m_total_score); forward_total: the sum
 * over the tokens alive after the last frame (:1389-1416, trailing epsilon arcs not added), what
 * get_total_log_likelihood returns.  pdf_occ [n_frames x pdfs] and tr_occ [transitions] follow the network's pdfs / trs
 * arrays and are written for AASR_FB_OK only; either may be NULL. */
aasr_status aasr_fb_batch_result(const aasr_fb_batch *b, int32_t u, int32_t *status, double *backward_total,
                                 double *forward_total, int32_t *attempts, double *pdf_occ, double *tr_occ);
/* After a sync, on a batch created with want_path: the emitting arc of each of utterance u's n_frames frames along the
 * best path, numbered as the network's emitting arcs are (csrc/hmmnet.h, aasr_hmmnet_arc_label); for an utterance that
 * was retried, the path of its last attempt.  The first call copies the whole batch's paths.  AASR_ERR_INVALID for an
 * utterance whose status is not AASR_FB_OK and for a batch made without want_path. */
aasr_status aasr_fb_batch_path(aasr_fb_batch *b, int32_t u, int32_t *arcs);
/* Diagnostic, read-only: the last aasr_fb_batch_dev call -- out[0] utterances launched, out[1] 1: node vectors in LDS,
 * 0: in global memory, out[2] LDS bytes of a workgroup, out[3] the attempt.  Four zeros before the first call. */
void aasr_debug_fb_shape(const aasr_fb_batch *b, int32_t *out);

/* The occupancies as weighted statistics entries, on the device (csrc/fb_entries.hip): what HmmNetBaumWelch::next_frame
 * (aku/HmmNetBaumWelch.cc:714-789) hands to the trainer.  Per frame s_t = sum_j occ[t][j] in the order of the network's
 * pdf list; an entry (t, j) exists where occ[t][j] > 0 and weighs occ[t][j] / s_t.  (The reference counts an arc whose
 * posterior underflowed to exactly 0 as an entry of weight 0; here it is none.)
 * After a sync, on a batch created with want_pdf_occ and device_occ; covers the AASR_FB_OK utterances only.  row0[u]: the
 * frame row of utterance u's first frame in the caller's frame buffer.  Entries are grouped by global pdf, ascending;
 * within a pdf the utterances come in batch order and the frames ascending -- for one pdf per frame the row list that
 * aasr_stats_accumulate_dev builds.  cnt (host, n_states + 1): cnt[s] is the first entry of pdf s, cnt[n_states] the number
 * of entries; it is the only thing copied back (one fetch, one wait).  *d_rows / *d_weights: device arrays of cnt[n_states]
 * elements owned by the batch, valid until the next call on it (NULL without entries), written on `stream`.  No atomics:
 * the same input gives the same bytes. */
aasr_status aasr_fb_batch_entries_dev(aasr_fb_batch *b, int32_t n_states, const int64_t *row0, void *stream, int64_t *cnt,
                                      const int32_t **d_rows, const double **d_weights);
/* After aasr_fb_batch_entries_dev: the entries copied to the host (rows / weights: as many elements as that call's
 * cnt[n_states]; either may be NULL), for callers that look at them rather than accumulate them.  Waits. */
aasr_status aasr_fb_batch_entries_host(aasr_fb_batch *b, int32_t *rows, double *weights);
/* After aasr_fb_batch_entries_dev: s_t of the frames of utterance u (n_frames doubles; the first call fetches every
 * utterance's).  AASR_ERR_INVALID for an utterance the entries do not cover. */
aasr_status aasr_fb_batch_frame_sums(aasr_fb_batch *b, int32_t u, double *sums);
/* Diagnostic, read-only: the last aasr_fb_batch_entries_dev call -- out[0] entries, out[1] utterances covered, out[2..4]
 * workgroups of the frame-sum, count and fill kernels.  Five zeros before the first call. */
void aasr_debug_fb_entries_shape(const aasr_fb_batch *b, int32_t *out);

/* The same entries grouped by frame, on the device (csrc/fb_frame_entries.hip): what the CMLLR accumulation walks
 * (aasr_mllr_accumulate_weighted_dev).  Preconditions as aasr_fb_batch_entries_dev: after a sync, on a batch created with
 * want_pdf_occ and device_occ; covers the AASR_FB_OK utterances only.  row0[u]: the frame row of utterance u's first frame
 * in the caller's frame buffer of n_rows rows; the utterances' rows must not overlap.  *d_off (n_rows + 1 offsets): the
 * entries of frame row r are d_off[r] .. d_off[r + 1]; a row that no covered utterance owns has none.  *d_pdf / *d_weight
 * (*n_entries elements): the global pdf and the weight occ[t][j] / s_t of every entry, a frame's entries in the order of
 * its network's pdf list (the order in which s_t is summed); s_t is the value of the pdf-major call, so a weight has the
 * same bytes in both.  The arrays are owned by the batch and valid until the next entries call of either kind on it (which
 * also replaces the other kind's entries).  The host fetches the number of entries only (one fetch, one wait), never the
 * offsets.  No atomics: the same input gives the same bytes. */
aasr_status aasr_fb_batch_frame_entries_dev(aasr_fb_batch *b, int32_t n_states, const int64_t *row0, int64_t n_rows,
                                            void *stream, int64_t *n_entries, const int64_t **d_off, const int32_t **d_pdf,
                                            const double **d_weight);
/* After aasr_fb_batch_frame_entries_dev: the three arrays copied to the host (off: that call's n_rows + 1 elements; pdf /
 * weight: its *n_entries; any may be NULL), for callers that look at them rather than accumulate them.  Waits.
 * aasr_fb_batch_frame_sums works after either entries call. */
aasr_status aasr_fb_batch_frame_entries_host(aasr_fb_batch *b, int64_t *off, int32_t *pdf, double *weight);
/* Diagnostic, read-only: the last aasr_fb_batch_frame_entries_dev call -- out[0] entries, out[1] utterances covered,
 * out[2..4] workgroups of the count, offset (first step) and fill kernels.  Five zeros before the first call. */
void aasr_debug_fb_frame_entries_shape(const aasr_fb_batch *b, int32_t *out);

/* logl main loop (aku/logl.cc:145-234) over one recipe slice (read with cluster_speakers): per utterance the sum of the
 * frame log-likelihoods along its .phn segmentation (aasr_segll; logl.cc's transtat is an unset global, so no
 * transition terms enter), or with hmmnet / den_hmmnet the forward total of the pass above over the recipe's hmmnet= /
 * den-hmmnet= network on the state rows of the model's scoring entry in the model's precision mode (AASR_PREC_F64:
 * double rows), frame limits from the line's start and end times (aku/Recipe.cc:223-228).  A failed backward pass is
 * run again with 2x ... 5x the backward beam (aku/logl.cc:183-199), new launches over the failed utterances only, with
 * the reference's warnings on stderr; an utterance that still fails is reported and skipped.  With info > 0 the
 * reference's "Log likelihood for file ..." line per utterance goes to stdout.  *total_log_likelihood: the sum.
 * Refused (AASR_ERR_UNSUPPORTED): mpv, recipe start-line / end-line, non-diagonal pools, model-side transforms. */
typedef struct aasr_logl_options {
  int32_t ophn;            /* -O: read the recipe's alignment= files                         */
  int32_t snl;             /* --snl: state-number labels                                     */
  int32_t hmmnet;          /* -H                                                             */
  int32_t den_hmmnet;      /* -D: the recipe's den-hmmnet= networks                          */
  int32_t mpv;             /* -M: refused                                                    */
  int32_t vit;             /* -V                                                             */
  int32_t ac_scale_given;  /* 1: -A was on the command line                                  */
  int32_t info;            /* -i                                                             */
  int32_t num_batches;     /* -B                                                             */
  int32_t batch_index;     /* -I                                                             */
  double fw_beam;          /* -F: 0 keeps the default 15 (set_pruning_thresholds)            */
  double bw_beam;          /* -W: 0 keeps the default 200                                    */
  double ac_scale;         /* -A                                                             */
  struct aasr_spkc *speakers; /* -S: the speaker configuration, or NULL                      */
} aasr_logl_options;
void aasr_logl_default_options(aasr_logl_options *opt);
aasr_status aasr_run_logl_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo, const char *recipe_path,
                                 const aasr_logl_options *opt, double *total_log_likelihood, aasr_run_stats *stats);

/* ---------------------------------------------------------------------------
 * Constrained MLLR estimation: aku/mllr.cc over state-segmented .phn files, one global transform per
 * speaker -- for a lin_transform feature module (-M) or as a model-side cmllr block (unitmode UNIT_NO).
 *
 * The accumulator of one model, on the device, for the CURRENT speaker: MllrTrainer::collect_data
 * (aku/MllrTrainer.cc:22-60, 147-163) for xi = [1, x]:
 *   G_i += sum_g (gamma_g / var_gi) xi xi^T,  k_i += sum_g (gamma_g mu_gi / var_gi) xi,  beta += sum_g gamma_g
 * with gamma_g = lik_g / sum lik (the mixture weights are not used, as in the reference; a frame whose sum is
 * 0 or not finite adds nothing).  Diagonal pools of 1 ... 63 dimensions (AASR_ERR_UNSUPPORTED beyond), the
 * unadapted model.  Deterministic: no atomics, fixed summation order. */
typedef struct aasr_mllr aasr_mllr;
aasr_status aasr_mllr_create(aasr_gmm *gmm, aasr_mllr **out);
void aasr_mllr_destroy(aasr_mllr *h);
/* zeroes the sums (the next speaker), enqueued on `stream` */
aasr_status aasr_mllr_reset(aasr_mllr *h, void *stream);
/* Adds n_frames double frame rows (device, [n_frames x dim]) whose pdfs are pdf[] (host; -1: skip) on
 * `stream`, no host wait.  Calls on one handle go to one stream. */
aasr_status aasr_mllr_accumulate_dev(aasr_mllr *h, const double *d_frames, int64_t n_frames,
                                     const int32_t *pdf, void *stream);
/* The same sums from weighted entries, all on the device (csrc/mllr_entries.hip): frame row t has the entries
 * d_off[t] .. d_off[t + 1] (d_off: n_frames + 1 ascending offsets into d_pdf / d_weight of n_entries elements, the
 * layout of aasr_fb_batch_frame_entries_dev).  Per frame, in list order, entry (pdf, p) adds p lik_g / sum_g lik_g per
 * Gaussian of the pdf's mixture (MllrTrainer::collect_data with the segmentator's probability, aku/mllr.cc:136-141) to
 * the frame's running weights and to beta; a value that is not > 0 adds nothing, an entry whose pdf is outside the model
 * is skipped, a frame without entries (or whose beta share is not > 0) adds nothing.  With one entry of weight 1.0 per
 * frame the accumulator gets the bytes of aasr_mllr_accumulate_dev with that pdf[]; both calls may be mixed on a handle.
 * d_off's last offset must not exceed n_entries (the caller's contract: the offsets are not fetched).  No host wait. */
aasr_status aasr_mllr_accumulate_weighted_dev(aasr_mllr *h, const double *d_frames, int64_t n_frames,
                                              const int64_t *d_off, const int32_t *d_pdf, const double *d_weight,
                                              int64_t n_entries, void *stream);
/* fetches the sums to the host (waits) */
aasr_status aasr_mllr_fetch(aasr_mllr *h, void *stream);
/* after a fetch: G [dim][dim + 1][dim + 1] (symmetric), k [dim][dim + 1], *beta; any pointer may be NULL */
aasr_status aasr_mllr_get(const aasr_mllr *h, double *G, double *k, double *beta);
/* MllTrainerComponent::calculate_transform (aku/MllrTrainer.cc:165-253) in double: W [dim][dim + 1],
 * column 0 the bias.  A zero pivot in a G_i or in A is AASR_ERR_INVALID.  Host only. */
aasr_status aasr_mllr_solve(int32_t dim, const double *G, const double *k, double beta, double *W);
/* MllrTrainer::calculate_transform(LinTransformModule *) (aku/MllrTrainer.cc:98-145): W as the float matrix
 * A [dim x dim] and bias b [dim] of a lin_transform module, composed with the module's old_A / old_b
 * (both NULL: the module has no transform yet) exactly as the reference composes them.  Host only. */
aasr_status aasr_mllr_compose(int32_t dim, const double *W, const float *old_A, const float *old_b,
                              float *A, float *b);

typedef struct aasr_mllr_options {
  int32_t ophn;         /* -O: read the recipe's alignment= files                          */
  int32_t info;         /* -i                                                              */
  int32_t num_batches;  /* -B                                                              */
  int32_t batch_index;  /* -I                                                              */
  double minframes;     /* -f (a tree's merge threshold; without a tree it changes nothing) */
  const char *module;   /* -M: the lin_transform module, or NULL for a model transform     */
  struct aasr_spkc *speakers; /* -S: the speaker configuration (required)                  */
  const char *out;      /* -o: the speaker file to write, or NULL                          */
} aasr_mllr_options;
void aasr_mllr_default_options(aasr_mllr_options *opt);

/* mllr main loop (aku/mllr.cc:213-332) over one recipe slice (read with cluster_speakers, sorted by
 * speaker): per speaker the features under its current configuration and the .phn segmentations, the
 * accumulation on the device, one solve, the transform set on the module / the cmllr block; the -i
 * messages on stderr and stdout; the speaker file.  seconds_device / seconds_copy_out stay 0. */
aasr_status aasr_run_mllr_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo,
                                 const char *recipe_path, const aasr_mllr_options *opt,
                                 aasr_run_stats *stats);

/* What the HMM networks add (aasr_run_mllr_networks_recipe).  A struct of its own: aasr_mllr_options stays as it is for
 * its callers. */
typedef struct aasr_mllr_network_options {
  int32_t networks;  /* 1: segment with the recipe's hmmnet= networks; 0: the call is aasr_run_mllr_recipe */
  int32_t viterbi;   /* --segmode vit: the best path instead of Baum-Welch                                  */
  double fw_beam;    /* -F: 0 keeps the default 15 (set_pruning_thresholds)                                 */
  double bw_beam;    /* -W: 0 keeps the default 200                                                         */
} aasr_mllr_network_options;
void aasr_mllr_network_default_options(aasr_mllr_network_options *opt);
/* The same loop with the recipe's hmmnet= networks in place of the .phn files (the reference's mllr -H,
 * aku/mllr.cc:73-145): per speaker and group of at most 2^18 frames the features under the speaker's current
 * configuration, the state rows of the model's scoring entry in the model's precision mode (in model mode: the unadapted
 * model's, the one the statistics are collected on), one forward-backward batch (aasr_fb_batch_*), the frame-major entries
 * (aasr_fb_batch_frame_entries_dev) and the weighted accumulation (aasr_mllr_accumulate_weighted_dev); fetch and solve
 * per speaker as in the .phn mode.  A failed backward pass is run again up to four times with 2x ... 5x the original
 * backward beam and the forward beam unchanged (aku/mllr.cc:87-102), new launches over the failed utterances only, with
 * the reference's messages on stderr; an utterance that still fails is reported and adds nothing.  The frame sums s_t are
 * checked as aasr_run_stats_networks_recipe checks them (the reference's warning above 0.02, AASR_ERR_INVALID where the
 * reference exits below 0.01, the largest |1 - s_t| on stderr at info > 0).  With info > 0 and a non-zero total, "Total
 * log likelihood: %f" on stderr: the sum of the forward totals of the utterances that ran.  A line without hmmnet= is the
 * reference's error.  Refused (AASR_ERR_UNSUPPORTED): opt->ophn.  net NULL or net->networks 0: aasr_run_mllr_recipe. */
aasr_status aasr_run_mllr_networks_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_topo *topo,
                                          const char *recipe_path, const aasr_mllr_options *opt,
                                          const aasr_mllr_network_options *net, aasr_run_stats *stats);

/* ---------------------------------------------------------------------------
 * LDA estimation: aku/lda.cc over state-segmented .phn files, or (aasr_run_lda_networks_recipe) over the recipe's HMM
 * networks.
 *
 * The class-scatter accumulator, on the device: FullStatisticsAccumulator::accumulate
 * (aku/Distributions.cc:133-141) per class c over many frames at once,
 *   gamma_c += w_t,  sum_x_c += w_t x_t,  sum_xx_c += w_t x_t x_t^T
 * on the FP64 matrix pipe (csrc/scatter_accum.hip; from weighted entries csrc/scatter_entries.hip).  1 ... 127
 * dimensions (AASR_ERR_UNSUPPORTED beyond).
 * Deterministic: no atomics, fixed summation order; the same calls give the same bytes. */
typedef struct aasr_scatter aasr_scatter;
aasr_status aasr_scatter_create(int32_t n_classes, int32_t dim, aasr_scatter **out);
void aasr_scatter_destroy(aasr_scatter *h);
/* Adds n_frames double frame rows (device, [n_frames x dim]) to the classes cls[] (host; -1: skip, any other value
 * outside 0 ... n_classes - 1: AASR_ERR_INVALID, nothing is added) with the weights d_weight (device, n_frames
 * doubles; NULL: 1) on `stream`, no host wait.  Calls on one handle go to one stream. */
aasr_status aasr_scatter_accumulate_dev(aasr_scatter *h, const double *d_frames, int64_t n_frames, const int32_t *cls,
                                        const double *d_weight, void *stream);
/* The same sums from weighted entries (csrc/scatter_entries.hip), so that a frame may stand under several classes: what
 * a Baum-Welch segmentation hands to the trainer.  cnt (host, n_classes + 1): cnt[c] is the first entry of class c,
 * cnt[n_classes] the number of entries -- the layout of aasr_stats_accumulate_weighted_dev and of
 * aasr_fb_batch_entries_dev.  d_rows / d_weights (device, cnt[n_classes] elements): entry e of class c adds
 * d_weights[e] xi xi^T for frame row d_rows[e] of d_frames ([n_frames x dim]; the rows must lie in 0 ... n_frames - 1, the
 * caller's contract: the list is not fetched).  An entry of weight 0 does not read its row: a NaN frame under weight 0
 * leaves the sums clean.  The host cuts cnt into work items of at most 256 entries of one class and uploads those
 * lists only; launches are cut by the slab bound exactly as in aasr_scatter_accumulate_dev, and the same input gives the
 * same bytes whatever the bound cuts the call into.  No host wait; the entry arrays must stay valid until the stream
 * is done with them.
 * Byte contract: with one entry per frame in the order of the row list that aasr_scatter_accumulate_dev builds (class
 * after class, frames ascending within a class) and entry weights equal to that call's per-row weights (or 1.0), the
 * accumulator has that call's bytes.  Both calls may be mixed on one handle.
 * AASR_ERR_INVALID, and nothing queued: cnt[0] != 0; a decreasing cnt; more than 2^31 entries or frames; entries
 * without frames, rows or weights. */
aasr_status aasr_scatter_accumulate_weighted_dev(aasr_scatter *h, const double *d_frames, int64_t n_frames,
                                                 const int64_t *cnt, const int32_t *d_rows, const double *d_weights,
                                                 void *stream);
/* fetches the sums to the host (waits) */
aasr_status aasr_scatter_fetch(aasr_scatter *h, void *stream);
/* after a fetch: gamma [n_classes], sum_x [n_classes x dim], sum_xx [n_classes x dim (dim + 1) / 2] -- the packed
 * lower triangle, row-major with j <= i, the order FullStatisticsAccumulator::dump_statistics writes; any pointer
 * may be NULL */
aasr_status aasr_scatter_get(const aasr_scatter *h, double *gamma, double *sum_x, double *sum_xx);
/* Diagnostic, read-only: out[0] the kernel's instance PB (16 PB >= dim + 1), out[1] work items and out[2] launches
 * of the last aasr_scatter_accumulate_dev or aasr_scatter_accumulate_weighted_dev call that had rows or entries to
 * add.  Zeros before the first. */
void aasr_debug_scatter_shape(const aasr_scatter *h, int32_t *out);
/* Diagnostic: the bound on a launch's slab memory in bytes (default 64 MiB, csrc/scatter.h; at least one item's
 * slab is always allowed), so that a test reaches several launches with a few thousand rows. */
aasr_status aasr_debug_scatter_set_slab_bytes(aasr_scatter *h, int64_t bytes);

/* lda.cc:380-446 in double, without LAPACK.  From the sums of the classes with selected[c] != 0, added in class
 * order: the data mean and covariance, B = sum min(gamma_c, max_gamma) (mu_c - mu)(mu_c - mu)^T and
 * W = sum min(gamma_c, max_gamma) Sigma_c; the target_dim leading eigenvectors of W^-1 B (from the
 * Cholesky-reduced symmetric problem, cyclic Jacobi), each of unit Euclidean length as dgeev returns them, as the
 * columns of P; lda = Lambda^-1/2 V^T P^T with (Lambda, V) the eigen-decomposition of P^T Sigma_data P, so that
 * lda Sigma_data lda^T = I.  lda is [target_dim x dim], row-major.
 * Row order and sign, which the reference leaves to LAPACK, are defined here: rows by DESCENDING eigenvalue of
 * the projected covariance P^T Sigma_data P, and every row's entry of largest magnitude (the first such) is
 * POSITIVE.
 * AASR_ERR_INVALID, and no matrix: fewer selected classes than target_dim + 1; a selected class without frames;
 * a W that is not positive definite; a projected covariance with a non-positive eigenvalue.  Host only. */
aasr_status aasr_lda_solve(int32_t n_classes, int32_t dim, const double *gamma, const double *sum_x,
                           const double *sum_xx, const int32_t *selected, double max_gamma, int32_t target_dim,
                           double *lda);
/* lda.cc:113-115, 247-263: which states get an accumulator.  The states by falling count -- a tie goes to the
 * LOWER state index (the reference's std::sort leaves it open) -- the first maxmem 10^6 / (8 dim^2) of them
 * (at most n_states) with count >= mingamma; then, when n_silence > 0, without the listed states.
 * selected [n_states] receives 0 / 1.  Host only. */
aasr_status aasr_lda_select(int32_t n_states, const double *count, double mingamma, int32_t maxmem, int32_t dim,
                            const int32_t *silence, int32_t n_silence, int32_t *selected);

typedef struct aasr_lda_options {
  int32_t ophn;         /* -O: read the recipe's alignment= files                       */
  int32_t info;         /* -i                                                           */
  int32_t target_dim;   /* -d: must equal the module's dimension                        */
  int32_t maxmem;       /* -m, in MB: caps the number of states with an accumulator     */
  int32_t no_silence;   /* --no-silence: without the states of _ and __                 */
  double mingamma;      /* --mingamma: minimum frame count of a state                   */
  double maxgamma;      /* --maxgamma: a state's weight in B and W is capped here       */
  const char *module;   /* -M: the lin_transform module                                 */
  const char *speakers; /* -S: path of a speaker configuration, or NULL                 */
  const char *out;      /* -w: the feature configuration to write, or NULL              */
  double *state_gamma;  /* NULL, or [aasr_topo_num_states]: receives the handle's gamma of every state */
  double seconds_scatter; /* out: device time of the scatter launches (events)          */
  double seconds_features; /* out: device time of the feature chain of pass 2 (events)  */
} aasr_lda_options;
void aasr_lda_default_options(aasr_lda_options *opt);

/* lda main loop (aku/lda.cc:143-463) over .phn segmentations.  feat_cfg_text: the feature configuration.
 * Before the device is opened: -M must name a lin_transform module whose configured `dim` equals -d.
 * Pass 1, host: per-state frame counts from the segmentations, frames past the feature end not counted
 * (lda.cc:228); the selection (aasr_lda_select).  Pass 2: the features AT THE MODULE'S SOURCE
 * (lda.cc:105-109, 226, 349) in double on the device under the speaker configuration, one scatter accumulation
 * per group of utterances with unselected states as class -1.  Then aasr_lda_solve; the matrix becomes the
 * module's transformation as LinTransformModule::set_transformation_matrix sets it (narrowed to float) and
 * the configuration is written to opt->out.  A missing _ or __ HMM is AASR_ERR_INVALID. */
aasr_status aasr_run_lda_recipe(const char *feat_cfg_text, const aasr_topo *topo, const char *recipe_path,
                                aasr_lda_options *opt, aasr_run_stats *stats);

/* What the HMM networks add (aasr_run_lda_networks_recipe).  A struct of its own: aasr_lda_options stays as it is for
 * its callers. */
typedef struct aasr_lda_network_options {
  int32_t networks;       /* 1: segment with the recipe's hmmnet= networks; 0: the call is aasr_run_lda_recipe */
  int32_t viterbi;        /* --segmode vit: the best path instead of Baum-Welch                                 */
  double fw_beam;         /* -F: 0 keeps the default 15 (set_pruning_thresholds)                                */
  double bw_beam;         /* -W: 0 keeps the default 200                                                        */
  int32_t ac_scale_given; /* 1: -A was on the command line                                                      */
  double ac_scale;        /* -A                                                                                 */
} aasr_lda_network_options;
void aasr_lda_network_default_options(aasr_lda_network_options *opt);
/* The host-side refusals of aasr_run_lda_networks_recipe, without opening the device, for a caller (the lda tool) that
 * wants them before it builds the model: recipe line limits; a line without hmmnet= (the reference's error); -d against
 * the module's configured dimension; a missing _ or __ HMM; opt->ophn (AASR_ERR_UNSUPPORTED); a lin_transform module
 * whose configuration gives no matrix (AASR_ERR_INVALID, the module named): the networks mode runs the whole chain to
 * score, so the model's input must exist. */
aasr_status aasr_lda_networks_check(const char *feat_cfg_text, const aasr_topo *topo, const char *recipe_path,
                                    const aasr_lda_options *opt);
/* lda over the recipe's hmmnet= networks: what aku/lda.cc:147-372 would compute from HmmNetBaumWelch's pdf_probs() with
 * -H.  The reference's own -H cannot run (the tool reads only --ph, so it has no Gaussians to score with, and asks an
 * option it never declares), so parity with the reference binary is unpinned; the yardstick is the restatement in
 * tools/lda_networks_restate.py.  gmm: the diagonal model that scores the chain's output (its dimension must be the
 * chain's: check_feature_dim).
 * aasr_lda_networks_check first.  Then per group of at most 1024 lines, 2^18 frames and 2^27 scores: the frames of the
 * chain's output; the state rows of the model's scoring entry in the model's precision mode; one forward-backward batch
 * (aasr_fb_batch_*), a failed backward pass run again up to four times with 2x ... 5x the backward beam (lda.cc:186-202)
 * with the reference's messages on stderr, an utterance that still fails reported and adding nothing; the frame sums
 * checked as aasr_run_stats_networks_recipe checks them; the pdf-major entries (aasr_fb_batch_entries_dev); the frames AT
 * THE MODULE'S SOURCE for the same utterances and frame ranges (the chain is evaluated twice per group), so that the
 * entries' row numbers address both buffers; one aasr_scatter_accumulate_weighted_dev over all states.
 * ONE pass, not the reference's two: the handle keeps every state's sums, a state's gamma is entry (0, 0) of them, and
 * the selection (aasr_lda_select, -m, --mingamma, --no-silence) is made on the fetched gamma.  That halves the
 * forward-backward work.  Under Baum-Welch a gamma that lies exactly at --mingamma could select differently from a sum
 * made in frame order; with net->viterbi the weights are 1.0 and gamma is exact.  Then aasr_lda_solve and the
 * configuration as in aasr_run_lda_recipe.  opt->state_gamma, seconds_scatter and seconds_features are filled as there.
 * With info > 0 the largest |1 - s_t| and the number of weighted entries on stderr.
 * net NULL or net->networks 0: aasr_run_lda_recipe (gmm may be NULL then). */
aasr_status aasr_run_lda_networks_recipe(const char *feat_cfg_text, aasr_gmm *gmm, const aasr_topo *topo,
                                         const char *recipe_path, aasr_lda_options *opt,
                                         const aasr_lda_network_options *net, aasr_run_stats *stats);

/* ---------------------------------------------------------------------------
 * Clustering of the Gaussian pool: aku/gcluster.cc in its default (diagonal) mode, one group.
 *
 * Every Gaussian is its mean and the diagonal of its covariance.  C centres start as the means of the first C
 * entries of a random permutation (libc rand() from seed 1, as a fresh process has it: the run entries call srand(1)
 * so that a call gives what the tool gives); every Gaussian goes to the centre of the nearest mean (Euclidean, all
 * centres); then four passes of: centre = mean of its members' means and covariances, every Gaussian to the valid
 * centre of the smallest Kullback-Leibler divergence.  A centre without members is invalid from then on.  The written
 * clusters are the valid ones, renumbered in order.
 *
 * The assignment passes and the centre sums run on the device (csrc/kl_cluster.hip) with the reference's own
 * operations in its own order -- no atomics, no reciprocal, no fused product -- so the result is the reference's map,
 * not one near it; log-determinants are summed on the host with the C library's log.  Any dimension >= 1. */

/* One assignment pass over plain host arrays: mean, cov [n_gauss x dim], ldet [n_gauss]; c_mean, c_cov
 * [n_clusters x dim], c_ldet, c_valid [n_clusters].  euclid != 0: out_dist = sqrt(sum_k (mean - c_mean)^2) over ALL
 * centres (cov, ldet, c_cov, c_ldet, c_valid are not read and may be NULL).  euclid == 0: out_dist =
 * (c_ldet - ldet + sum_k (cov + (mean - c_mean)^2) / c_cov - dim) / 2 over the centres with c_valid != 0.
 * out_index [n_gauss]: the first centre of the smallest distance below 1e100, or 0 (out_dist 1e100) when there is
 * none -- also when centre 0 is invalid, as in the reference. */
aasr_status aasr_gcluster_assign(int32_t dim, int32_t n_gauss, const double *mean, const double *cov, const double *ldet,
                                 int32_t n_clusters, const double *c_mean, const double *c_cov, const double *c_ldet,
                                 const int32_t *c_valid, int32_t euclid, int32_t *out_index, double *out_dist);
/* compute_cluster_statistics: per cluster the sums of its members' (map [n_gauss], every entry in
 * 0 ... n_clusters - 1) means and covariances in Gaussian order, times 1 / count; c_valid = count > 0;
 * c_ldet = sum_k log(c_cov) on the host.  A cluster without members gets zeros. */
aasr_status aasr_gcluster_centres(int32_t dim, int32_t n_gauss, const double *mean, const double *cov, int32_t n_clusters,
                                  const int32_t *map, double *c_mean, double *c_cov, double *c_ldet, int32_t *c_valid);
/* Diagnostic: the number of centres the assignment kernel walks at a time (its tie rule has to hold across them). */
int32_t aasr_debug_gcluster_chunk(void);

typedef struct aasr_gcluster_options {
  int32_t clusters;     /* -C: at least 2, at most the number of Gaussians                          */
  int32_t iterations;   /* -t: below 1 is an error; the single-group run makes four passes whatever it says */
  int32_t info;         /* -i: 1 the iterations' average divergence and the count written, 2 every Gaussian */
  int32_t full;         /* -F given: full-covariance centres, AASR_ERR_UNSUPPORTED                  */
  int32_t progress;     /* the tool's "make initial clusters" / "start clustering" lines on stderr  */
  const char *regtree;  /* -R, or NULL; with base: per-class groups, AASR_ERR_UNSUPPORTED           */
  const char *base;     /* -b, or NULL                                                              */
  int32_t written;      /* out: clusters written (the valid ones)                                   */
  double seconds_steps; /* out: host clock around the five assignment + centre steps, each to its synchronisation */
} aasr_gcluster_options;
void aasr_gcluster_default_options(aasr_gcluster_options *opt);
/* gcluster's main: reads gk_path (any pool the engine reads; full-covariance and subspace Gaussians by their
 * covariance diagonal), clusters, writes out_path ("n\n" then "gaussian cluster\n" per Gaussian).  The reference's
 * errors with its messages, all before the device is opened: "Invalid number of clusters", "Invalid number of
 * iterations", "Both tree and model must be given", "Not enough Gaussians to cluster!". */
aasr_status aasr_run_gcluster(const char *gk_path, const char *out_path, aasr_gcluster_options *opt);
/* The same run on plain arrays: cluster_of [n_gauss] receives the renumbered cluster of every Gaussian. */
aasr_status aasr_gcluster_arrays(int32_t dim, int32_t n_gauss, const double *mean, const double *cov,
                                 aasr_gcluster_options *opt, int32_t *cluster_of);
/* The same run on a loaded model's Gaussians; the result is installed as aasr_gmm_read_clustering installs the file
 * the tool would have written (its reader's last pair counted twice included). */
aasr_status aasr_gmm_cluster(aasr_gmm *h, int32_t n_clusters, int32_t info);

/* ---------------------------------------------------------------------------
 * Feature normalization and PCA: aku/feanorm.cc.
 *
 * The blocked moments, on the device (csrc/moments_accum.hip).  A SEGMENT is a contiguous run of rows of a frame
 * buffer -- feanorm's block of -b frames inside one utterance.  Per segment, in double:
 *   AASR_MOMENTS_DIAG: the count, sum x and sum x^2 (vector pipe), any dimension >= 1;
 *   AASR_MOMENTS_FULL: the count, sum x and sum x x^T (FP64 matrix pipe), 1 ... 127 dimensions
 *                      (AASR_ERR_UNSUPPORTED beyond).
 * Deterministic: no atomics; a segment's sums depend on its rows alone, not on the calls and launches around it. */
#define AASR_MOMENTS_DIAG 0
#define AASR_MOMENTS_FULL 1
typedef struct aasr_moments aasr_moments;
aasr_status aasr_moments_create(int32_t dim, int32_t mode, aasr_moments **out);
void aasr_moments_destroy(aasr_moments *h);
/* Appends n_segments segments of the double frame rows d_frames (device, [n_frames x dim]) on `stream`, no host
 * wait.  segments (host): [n_segments x 3] = first row, length (>= 1), utterance (any number, handed back by
 * aasr_moments_get); a segment outside the buffer is AASR_ERR_INVALID and nothing is added.  Calls on one handle go
 * to one stream. */
aasr_status aasr_moments_accumulate_dev(aasr_moments *h, const double *d_frames, int64_t n_frames,
                                        const int32_t *segments, int32_t n_segments, void *stream);
/* waits until the sums of every segment given so far are on the host */
aasr_status aasr_moments_fetch(aasr_moments *h, void *stream);
int64_t aasr_moments_num_segments(const aasr_moments *h);
/* after a fetch, per segment in the order given: count [n], utterance [n], sum_x [n x dim] and sum_xx --
 * DIAG: [n x dim], sum x^2; FULL: [n x dim (dim + 1) / 2], the packed lower triangle of sum x x^T, row-major with
 * j <= i.  Any pointer may be NULL. */
aasr_status aasr_moments_get(const aasr_moments *h, double *count, int32_t *utterance, double *sum_x, double *sum_xx);
/* feanorm.cc:181-242 on the host, after a fetch, over the segments in the order given: sums += segment / block_size
 * and count += length / block_size in double (the division is by block_size whatever the segment's length).
 * keep [n] or NULL: a segment with keep == 0 is left out.  count [1], sum_x [dim], sum_xx as in aasr_moments_get
 * for one segment. */
aasr_status aasr_moments_blocked(const aasr_moments *h, int32_t block_size, const int32_t *keep, double *count,
                                 double *sum_x, double *sum_xx);
/* Diagnostic, read-only: out[0] the full-mode kernel's instance PB (16 PB >= dim + 1; 0 in diagonal mode), out[1]
 * work items and out[2] launches of the last aasr_moments_accumulate_dev call.  Zeros before the first. */
void aasr_debug_moments_shape(const aasr_moments *h, int32_t *out);
/* Diagnostic: at most n segments a launch (default: what csrc/moments.h allows), so that a test reaches several
 * launches with a few segments. */
aasr_status aasr_debug_moments_set_launch_segments(aasr_moments *h, int32_t n);

/* feanorm.cc:281-325 in double, without LAPACK (the cyclic Jacobi solver of the lda driver).  cov [dim x dim]
 * symmetric, row-major; scale [dim], the normalization's scale (NULL: ones).  pca [dim x dim], row-major:
 * row i = eigenvector i of cov, then
 *   unit_determinant == 0:  pca(i, j) /= sqrt(eigenvalue i), then pca(i, j) /= scale[j]   (unit variance)
 *   unit_determinant != 0:  pca(i, j) /= scale[j], then pca /= |det pca|^(1 / dim)        (unit determinant)
 * Row order and sign, which the reference leaves to LAPACK, are defined here: rows by ASCENDING eigenvalue, as dsyev
 * returns them (a tie: the solver's lower index), and every row's entry of largest magnitude (the first such) is
 * POSITIVE.  eigenvalues: NULL or [dim], ascending.  A non-positive (or NaN) eigenvalue is AASR_ERR_INVALID and no
 * matrix, in both branches.  Host only. */
aasr_status aasr_feanorm_pca(int32_t dim, const double *cov, const double *scale, int32_t unit_determinant, double *pca,
                             double *eigenvalues);

typedef struct aasr_feanorm_options {
  int32_t info;             /* -i                                                                   */
  int32_t block_size;       /* -b: frames per block (1000)                                          */
  int32_t cov;              /* --cov: estimate and print the covariance                             */
  int32_t print;            /* -p: print mean and variance                                          */
  int32_t unit_determinant; /* -u                                                                   */
  const char *module;       /* -M: the normalization module, or NULL                                */
  const char *pca;          /* -P: the lin_transform module that receives the PCA, or NULL          */
  const char *speakers;     /* -S: path of a speaker configuration, or NULL                         */
  const char *utt;          /* --utt: the speaker file to write, or NULL                            */
  const char *out;          /* -w: the feature configuration to write, or NULL                      */
  double blocks;            /* out: the global count (blocks, the tail of an utterance a fraction)  */
  double seconds_moments;   /* out: device time of the moment launches (events)                     */
  double seconds_features;  /* out: device time of the feature chain (events)                       */
} aasr_feanorm_options;
void aasr_feanorm_default_options(aasr_feanorm_options *opt);

/* feanorm's main (aku/feanorm.cc:65-386).  feat_cfg_text: the feature configuration; the recipe is read without
 * batching.  Before the device is opened: the reference's refusals with its messages ("Module %s is not a
 * normalization module", "--utt requires the normalization module (--module)", "Module %s is not a linear
 * transformation module", "--utt requires --speakers", "unknown module requested: %s"), its warning for -w without
 * -M, a -P module whose source's dimension is not the statistics' (the reference asserts), a block size below 1 and,
 * with --cov or -P, more than 127 dimensions (AASR_ERR_UNSUPPORTED).
 * Per recipe line: -S's set_speaker / set_utterance, the frames (int)(start-time rate) ... (int)(end-time rate)
 * (0: to the end) of the -M module's FIRST SOURCE (without -M: of the chain's output) in double on the device, cut
 * into blocks of block_size; the blocks' moments on the device, the blocked sums on the host in recipe order.  The
 * trailing partial block of an utterance enters the global sums only when the input's end stopped the loop, not
 * when end-time did (feanorm.cc:178-195); --utt counts it either way.  With --utt the utterances go to the device
 * one at a time, since every utterance's normalization is set on the module before the next line's speaker change
 * reads the module back.  Then mean = sum / count, scale = 1 / sqrtf(sum2 / count - mean^2), aasr_feanorm_pca;
 * -p / --cov print to stdout ("%f "); --utt writes the speaker file (every speaker and utterance); the
 * normalization (without --utt) and the PCA are set on their modules and -w writes the configuration. */
aasr_status aasr_run_feanorm_recipe(const char *feat_cfg_text, const char *recipe_path, aasr_feanorm_options *opt,
                                    aasr_run_stats *stats);

/* ---------------------------------------------------------------------------
 * Model re-estimation from statistics dumps: aku/estimate.cc --ml over diagonal pools.
 *
 * The estimation handle, host only: a model's .gk / .mc / .ph files with the accumulators that the dumps of stats
 * (.gks, .mcs, .phs, .lls) are added to.  Pools with full-covariance or subspace Gaussians are
 * AASR_ERR_UNSUPPORTED.  State s emits mixture s; the transitions are numbered in state order, as HmmSet numbers
 * them. */
typedef struct aasr_estimate aasr_estimate;
aasr_status aasr_estimate_create(const char *gk, const char *mc, const char *ph, aasr_estimate **out);
void aasr_estimate_destroy(aasr_estimate *h);
/* Adds base.gks and base.mcs, base.phs when transitions != 0, and the lines of base.lls, in double
 * (HmmSet::accumulate_{gk,mc,ph}_from_dump, aku/HmmSet.cc:655-765).  The first dump's mode word fixes the accumulator
 * kind for the handle's life: 1 diagonal second moments, 3 the packed lower triangle (PDF_ML_FULL_STATS); a mode with
 * discriminative bits is AASR_ERR_UNSUPPORTED.  The reference's errors, with its messages: a wrong pool size,
 * dimension, pdf count or transition count, a negative feacount, a pdf index outside the pool, a transition that
 * cannot be found.  A missing .phs is only a message on stderr; a .phs that ends before its first line is allowed,
 * and one that ends later repeats its last line up to the announced count, as the reference's reader does. */
aasr_status aasr_estimate_add_dump(aasr_estimate *h, const char *base, int32_t transitions);
/* --minvar (0.1) and --covsmooth (0; without effect on diagonal Gaussians) */
aasr_status aasr_estimate_set_gaussian_parameters(aasr_estimate *h, double minvar, double covsmooth);
/* HmmSet::estimate_transition_parameters (aku/HmmSet.cc:782-815): per state the counts over their FLOAT running sum,
 * floored at 0.001; a state without counts keeps its probabilities.  Nothing happens before the first .phs. */
aasr_status aasr_estimate_transitions(aasr_estimate *h);
/* The ML update.  pool != 0: per Gaussian mean = sum_x (1 / gamma), variance = sum_xx_i / gamma - mean_i mean_i
 * (mode 3: the diagonal of sum_xx (1 / gamma) - mean mean^T), floored at minvar; mixtures != 0: per state's mixture
 * weight_k = gamma_k / sum gamma.  A Gaussian or mixture without statistics keeps its parameters and gets the
 * reference's warning on stderr. */
aasr_status aasr_estimate_ml(aasr_estimate *h, int32_t pool, int32_t mixtures);
/* The pool edits (aku/HmmSet.cc:1058-1350).  index_map: NULL or [pool size before the call], the Gaussian's new index
 * or -1.  Where the reference's std::sort leaves Gaussians of equal occupancy in any order, the lower index goes
 * first. */
aasr_status aasr_estimate_delete_gaussians(aasr_estimate *h, double minocc, int32_t *index_map, int32_t *n_deleted);
aasr_status aasr_estimate_remove_mixture_components(aasr_estimate *h, double min_weight, int32_t *index_map,
                                                    int32_t *n_deleted);
aasr_status aasr_estimate_split_gaussians(aasr_estimate *h, double minocc, int32_t maxmixgauss, int32_t numgauss,
                                          double splitalpha, int32_t *n_splits);
/* PDFPool::write_gk, HmmSet::write_mc, HmmSet::write_legacy_ph: six significant digits ("%g") */
aasr_status aasr_estimate_write_gk(const aasr_estimate *h, const char *path);
aasr_status aasr_estimate_write_mc(const aasr_estimate *h, const char *path);
aasr_status aasr_estimate_write_ph(const aasr_estimate *h, const char *path);
/* out[7]: Gaussians, dimension, mixtures, mixture components, states, transitions, statistics mode (0: no dump yet) */
void aasr_estimate_sizes(const aasr_estimate *h, int32_t *out);
/* The accumulated statistics.  Per Gaussian: accumulated [G] (0 / 1), feacount [G], gamma [G], sum_x [G x dim],
 * sum_xx [G x dim] (mode 1) or [G x dim (dim + 1) / 2] (mode 3, row-major with j <= i).  Per mixture: accumulated [M],
 * offsets [M + 1] into gamma [components].  Per transition: accumulated [T], occupancy [T].  Any pointer may be NULL. */
aasr_status aasr_estimate_get_statistics(const aasr_estimate *h, int32_t *accumulated, int32_t *feacount, double *gamma,
                                         double *sum_x, double *sum_xx);
aasr_status aasr_estimate_get_mixture_statistics(const aasr_estimate *h, int32_t *accumulated, int32_t *offsets,
                                                 double *gamma);
aasr_status aasr_estimate_get_transition_statistics(const aasr_estimate *h, int32_t *accumulated, double *occupancy);
/* The current parameters: mean, var [G x dim]; offsets [M + 1], index and weight [components]; source, target (offset
 * relative to the source's place in its HMM) and prob [T].  Any pointer may be NULL. */
aasr_status aasr_estimate_get_gaussians(const aasr_estimate *h, double *mean, double *var);
aasr_status aasr_estimate_get_mixtures(const aasr_estimate *h, int32_t *offsets, int32_t *index, double *weight);
aasr_status aasr_estimate_get_transitions(const aasr_estimate *h, int32_t *source, int32_t *target, double *prob);

/* MLLT (HmmSet::estimate_mllt, aku/HmmSet.cc:841-1056) on the device (csrc/mllt.hip).  The handle builds the
 * covariances S_g = sum_xx_g (1 / gamma_g) - mean_g mean_g^T once and keeps them resident in double.  gamma [G],
 * sum_x [G x dim], sum_xx [G x dim (dim + 1) / 2] packed lower triangles; accumulated [G] or NULL (all): a Gaussian
 * with 0 is skipped everywhere (zero covariance, zero weight).  1 ... 63 dimensions (AASR_ERR_UNSUPPORTED beyond).
 * Deterministic: no atomics; the same input gives the same bytes, whatever the slab bound cuts a call into. */
typedef struct aasr_mllt aasr_mllt;
aasr_status aasr_mllt_create(int32_t dim, int64_t n_gauss, const double *gamma, const double *sum_x, const double *sum_xx,
                             const int32_t *accumulated, aasr_mllt **out);
void aasr_mllt_destroy(aasr_mllt *h);
/* the resident covariances, [G x dim (dim + 1) / 2] packed lower triangles */
aasr_status aasr_mllt_get_covariances(aasr_mllt *h, double *cov);
/* var [G x dim]: var_gi = a_i S_g a_i^T for the rows a_i of A [dim x dim], not floored */
aasr_status aasr_mllt_variances(aasr_mllt *h, const double *A, double *var);
/* g_sums [dim x dim (dim + 1) / 2]: the packed lower triangle of sum_g (gamma_g / var_gi) S_g for every i, on the FP64
 * matrix pipe */
aasr_status aasr_mllt_g_sums(aasr_mllt *h, const double *var, double *g_sums);
/* Host only: `iterations` inner updates of A [dim x dim] (aku/HmmSet.cc:955-980).  Each takes the cofactors
 * C = |det A| (A^T)^-1 of the current A once and then replaces EVERY row from them: row_i = G_i^T c_i, scaled by
 * sqrt(beta / c_i . row_i).  g_inv [dim x dim x dim]: the inverted G_i, row-major. */
aasr_status aasr_mllt_update_rows(int32_t dim, const double *g_inv, double beta, int32_t iterations, double *A);
/* The whole loop from A = I: 7 times (variances floored at minvar, G sums, their inverses, 80 inner updates,
 * A / |det A|^(1 / dim)), then mean [G x dim] = A mean_g and var [G x dim] = the floored variances under the final A;
 * rows of skipped Gaussians are left as they are.  mean and var may be NULL. */
aasr_status aasr_mllt_estimate(aasr_mllt *h, double minvar, double *A, double *mean, double *var);
/* Diagnostic, read-only: out[0] the kernels' instance PB (16 PB >= dim), out[1] work items and out[2] launches of the
 * last aasr_mllt_g_sums pass.  Zeros before the first. */
void aasr_debug_mllt_shape(const aasr_mllt *h, int32_t *out);
/* Diagnostic: out[4] = seconds (host clock, transfers included) of the covariance build, of all variance passes, of
 * all G passes and of the host solves so far. */
void aasr_debug_mllt_times(const aasr_mllt *h, double *out);
/* Diagnostic: the bound on a launch's slab memory in bytes (default 64 MiB, csrc/mllt.h; at least one item's slab is
 * always allowed). */
aasr_status aasr_debug_mllt_set_slab_bytes(aasr_mllt *h, int64_t bytes);
/* estimate --mllt on a handle whose dumps are mode 3 (AASR_ERR_INVALID otherwise, naming stats --mllt): the loop
 * above over the handle's statistics, the new means and variances into the pool, the mixtures as in the ML update.
 * old_matrix [dim x dim] or NULL (identity); new_matrix [dim x dim] = A old_matrix in float.  seconds: NULL or [4],
 * as aasr_debug_mllt_times. */
aasr_status aasr_estimate_run_mllt(aasr_estimate *h, const float *old_matrix, float *new_matrix, double *seconds);

typedef struct aasr_estimate_options {
  const char *gk, *mc, *ph;     /* the previous model (-b, or -g / -m / -p)                            */
  const char *base_name;        /* what --savesum prints: -b's value, or the .gk path (NULL)           */
  const char *config;           /* -c: path of the feature configuration, or NULL                      */
  const char *list;             /* -L: file with one dump base name per line                           */
  const char *out;              /* -o: base name of the output model                                   */
  const char *mllt;             /* --mllt: the lin_transform module, or NULL                           */
  const char *savesum;          /* -s: the summary file to append to, or NULL                          */
  int32_t transitions;          /* -t                                                                  */
  int32_t info;                 /* -i                                                                  */
  double minvar;                /* --minvar (0.1)                                                      */
  double covsmooth;             /* --covsmooth (0)                                                     */
  int32_t delete_set;           /* --delete given                                                      */
  double delete_minocc;         /* --delete                                                            */
  int32_t mremove_set;          /* --mremove given                                                     */
  double mremove;               /* --mremove                                                           */
  int32_t split;                /* --split                                                             */
  int32_t minocc_set;           /* --minocc given                                                      */
  double minocc;                /* --minocc (0)                                                        */
  int32_t maxmixgauss;          /* --maxmixgauss (0)                                                   */
  int32_t numgauss_set;         /* --numgauss given                                                    */
  int32_t numgauss;             /* --numgauss (-1)                                                     */
  double splitalpha;            /* --splitalpha (1)                                                    */
  int32_t no_mixture_update;    /* --no-mixture-update                                                 */
  int32_t no_write;             /* --no-write                                                          */
  int32_t n_deleted;            /* out: Gaussians deleted by --delete                                  */
  int32_t n_removed;            /* out: Gaussians deleted by --mremove                                 */
  int32_t n_splits;             /* out: Gaussians split                                                */
  double seconds_read;          /* out: reading and adding the dumps                                   */
  double seconds_mllt;          /* out: the MLLT estimation, configuration load included               */
  double seconds_mllt_parts[4]; /* out: as aasr_debug_mllt_times                                       */
} aasr_estimate_options;
void aasr_estimate_default_options(aasr_estimate_options *opt);

/* estimate's main (aku/estimate.cc:158-425) for --ml.  In this order: "Either --minocc or --numgauss is required with
 * --split"; "Must specify configuration file with MLLT"; the model; with --mllt, before any dump is read and before
 * the device is opened: "Module %s is not a transform module", a module whose matrix is not dim x dim, more than 63
 * dimensions (AASR_ERR_UNSUPPORTED); the dumps of the list in order; with --mllt, dumps that are not mode 3 are
 * refused (the reference would invert a zero matrix).  Then the transitions (-t), the ML update or MLLT, --delete,
 * --mremove, --split, the writers (out.mc, out.ph, out.gk; out.cfg with -c) and the summary, appended with 12 digits.
 * --no-write writes nothing.  The device is opened only for --mllt and for writing out.cfg (the configuration writer
 * belongs to the feature handle); --ml without -c runs on a machine without one. */
aasr_status aasr_run_estimate(aasr_estimate_options *opt);

/* ---------------------------------------------------------------------------
 * Decision-tree state tying: aku/tie.cc over aku/PhonePool.cc.
 *
 * A CONTEXT PHONE is a label ("a-b+c", "x-a-b+c+y", "b") with a state number; its class index is the order of its
 * first mention.  Per class the handle keeps the raw sums gamma, sum x, sum x x^T as one row on the device; a
 * cluster's statistic is the sum of its members' rows (csrc/tie.h).  One tree per centre phone and state is grown by
 * the rules of the rule file; candidates are chosen on the host (frame counts are integers), their sums and
 * likelihood gains come from the device (csrc/tie_split.hip), the winner is picked on the host with the reference's
 * strict comparisons in the reference's order (rule outer, context index inner).  A covariance that is not positive
 * definite is no special case: the plain column Cholesky yields NaN or an infinity and the comparisons do what they do.
 *
 * 1 ... 63 dimensions (AASR_ERR_UNSUPPORTED beyond: one d x d matrix of doubles has to fit 32 KiB of LDS).
 * Parity with the reference binary is not pinned: no reference tie is built (it needs LAPACK++). */
typedef struct aasr_tie aasr_tie;
/* PhonePool::center_phone / fill_left_contexts / fill_right_contexts: text (aasr_free) = "centre\nleft\nright", the
 * contexts nearest first and separated by \x1f.  Host only. */
aasr_status aasr_tie_parse_label(const char *label, char **text, int64_t *len);
/* Reads the rule file ("NAME context p1,p2,..." per line, the type in any letter case); the reference's messages for
 * a short line, an unknown type and a rule without phones.  Host only. */
aasr_status aasr_tie_create(int32_t dim, const char *rule_path, aasr_tie **out);
void aasr_tie_destroy(aasr_tie *h);
int32_t aasr_tie_num_rules(const aasr_tie *h);
int32_t aasr_tie_num_classes(const aasr_tie *h);
/* text (aasr_free): per rule "NAME\x1fphone\x1fphone...\n", the phones in set order */
aasr_status aasr_tie_rules_text(const aasr_tie *h, char **text, int64_t *len);
/* PhonePool::get_context_phone: the class of (label, state), new or known.  Refused once statistics are set.  Host only. */
aasr_status aasr_tie_context_phone(aasr_tie *h, const char *label, int32_t state, int32_t *cls);
/* The classes' statistics from host arrays in aasr_scatter_get's layout (gamma [C], sum_x [C x dim], sum_xx
 * [C x dim (dim + 1) / 2]), uploaded as rows.  They must be finite. */
aasr_status aasr_tie_set_stats(aasr_tie *h, const double *gamma, const double *sum_x, const double *sum_xx);
/* The kernel pair on caller-given lists.  Job j: job_k[j] classes (its slice of idx, any order) and job_rows[j] masks
 * over that list, (job_k[j] + 31) / 32 words each, bit k % 32 of word k / 32 for list position k; the jobs' lists and
 * masks follow each other in idx and mask.  Output row = sum of the listed classes' rows whose bit is set; the jobs'
 * rows are numbered through.  sums (or NULL): [rows x E], E = 1 + dim + dim (dim + 1) / 2 = [gamma, sum x, packed
 * lower triangle].  Candidate c = cands[3 c ...] = (parent row, child 1 row, child 2 row or -1 for parent - child 1);
 * gain [n_cands] = (gamma_p ld_p - gamma_1 ld_1 - gamma_2 ld_2) / 2 with ld = 2 sum log L_ii of the side's
 * covariance.  Same input, same bytes. */
aasr_status aasr_tie_evaluate(aasr_tie *h, int32_t n_jobs, const int32_t *job_k, const int32_t *job_rows, const int32_t *idx,
                              const uint32_t *mask, double *sums, int32_t n_cands, const int32_t *cands, double *gain);
/* PhonePool::decision_tree_cluster_context_phones: min_count --count, sgain --sgain, max_context --context (<= 0: every
 * context index the phone has).  hops 2: members -> sums per (context index, label) -> candidates; hops 1: members ->
 * candidates.  One launch sequence per round of all trees. */
aasr_status aasr_tie_split(aasr_tie *h, int32_t min_count, double sgain, int32_t max_context, int32_t hops, int32_t info);
/* PhonePool::merge_context_phones with --mloss. */
aasr_status aasr_tie_merge(aasr_tie *h, double mloss, int32_t info);
/* The clusters in their final order (the state numbering), text (aasr_free): per cluster
 * "phone\x1fstate\x1fstate index\x1foccupancy\x1fclass,class,...\x1frule:context:answer,...|rule:context:answer,...\n"
 * -- the rule sets a merge has joined are separated by '|'. */
aasr_status aasr_tie_clusters_text(aasr_tie *h, char **text, int64_t *len);
/* PhonePool::save_to_basebind, byte for byte: phones whose label starts with '_' (and every phone with max_context <=
 * 0) plain, the others as the full product of the context set, "label n s1 ... sn\n".  Host only. */
aasr_status aasr_tie_basebind_text(aasr_tie *h, int32_t max_context, char **text, int64_t *len);
aasr_status aasr_tie_write_basebind(aasr_tie *h, const char *path, int32_t max_context);
/* PhonePool::save_model: base.mc, base.ph, base.gk in HmmSet::write_all's text formats -- one full-covariance Gaussian
 * per tied state (mu = sum x / gamma, Sigma = sum x x^T / gamma - mu mu^T of the cluster's summed row), mixture
 * "1 s 1", transitions 0: 0.8 and 1: 0.2. */
aasr_status aasr_tie_write_model(aasr_tie *h, const char *base, int32_t max_context);
/* Diagnostics.  The occupancies alone (no device), and the split loop with gains from the caller: fn is called per
 * candidate with the cluster's classes and the new set's classes, both ascending.  out[6] of the shape: work items of
 * the first and second hop, sides and candidates of the last batch, rounds of the last split and merge. */
typedef double (*aasr_tie_gain_fn)(void *user, int32_t n_members, const int32_t *members, int32_t n_set, const int32_t *set);
aasr_status aasr_debug_tie_set_occupancy(aasr_tie *h, const double *gamma);
aasr_status aasr_debug_tie_split_given(aasr_tie *h, int32_t min_count, double sgain, int32_t max_context, aasr_tie_gain_fn fn,
                                       void *user);
void aasr_debug_tie_shape(const aasr_tie *h, int32_t *out);

typedef struct aasr_tie_options {
  int32_t ophn;        /* -O: the recipe's alignment field names the .phn                       */
  int32_t hmmnet;      /* -H given: "This feature is currently broken. Fix it?", as the reference */
  int32_t info;        /* -i                                                                    */
  int32_t count;       /* --count (100)                                                         */
  int32_t context;     /* --context (1)                                                         */
  int32_t mloss_given; /* --mloss given: merge after the split                                  */
  int32_t hops;        /* 2 (default) or 1, as aasr_tie_split                                   */
  int32_t clusters;    /* out: tied states                                                      */
  double sgain;        /* --sgain (0)                                                           */
  double mloss;        /* --mloss (0)                                                           */
  const char *rule;    /* -u                                                                    */
  const char *speakers; /* -S, or NULL                                                          */
  const char *out;      /* -o, or NULL                                                          */
  const char *basebind; /* -B, or NULL: exactly one of out and basebind                         */
  double seconds_scatter, seconds_features, seconds_split, seconds_merge; /* out */
} aasr_tie_options;
void aasr_tie_default_options(aasr_tie_options *opt);
/* tie's main (aku/tie.cc:137-280) over .phn files.  Host only and in this order: -H's message; the recipe; "Specify
 * either --out or --basebind for output"; recipe line limits (AASR_ERR_UNSUPPORTED); the rule file; a text pass over
 * the .phn files that numbers every (label, state) ("Context phone tying requires phn files with state numbers!", here
 * also for a line past the feature end, which the reference never reads).  Then the device: more than 63 dimensions is
 * AASR_ERR_UNSUPPORTED before any frame is read; per line the context phone (first label, state) comes to exist and the
 * frames start ... end - 1 go to its class through aasr_scatter_accumulate_dev; the line that meets the feature end is
 * the file's last, with the frames it has before the end or none; the sums stay on the device for the split, the merge (with mloss_given) and the
 * writer.  A frame that two lines of one file claim is AASR_ERR_UNSUPPORTED. */
aasr_status aasr_run_tie_recipe(const char *feat_cfg_text, const char *recipe_path, aasr_tie_options *opt, aasr_run_stats *stats);

/* ---------------------------------------------------------------------------
 * State duration models: aku/dur_est.cc over state-numbered .phn files (what stats --networks -M vit -a writes).  Host
 * only: no device is opened. */
typedef struct aasr_dur_est_options {
  int32_t ophn;       /* -O: read the recipe's alignment= files            */
  int32_t maxdur;     /* -M (100): longer durations count as this          */
  int32_t skip;       /* --skip (0): the first states get no model         */
  int32_t mincount;   /* --mincount (10)                                   */
  int32_t info;       /* -i                                                */
  const char *hist;   /* --hist: the histogram file to write, or NULL      */
  const char *gamma;  /* --gamma: the .dur file to write, or NULL          */
} aasr_dur_est_options;
void aasr_dur_est_default_options(aasr_dur_est_options *opt);
/* dur_est's main (aku/dur_est.cc:142-218).  The reader runs at PhnReader's default frame rate of 125 (Recipe.cc:158, no
 * feature configuration), with the line's start-time / end-time and start-line / end-line as PhnReader applies them
 * (PhnReader.cc:83-124; a start-line past the file's end or past end-line, where the reference never returns, ends the
 * file's lines).  init_utterance_segmentation consumes a file's first line; every later line adds end - start frames
 * (capped at maxdur) to the histogram of the state `state` of the HMM `label`.  A line without a state number is
 * "Collecting duration statistics requires phn files with state numbers!"; an unknown label, a state the HMM does not
 * have, or a line of no frames (where the reference indexes out of its tables) is AASR_ERR_INVALID.  A file without
 * lines gives the reference's two messages on stderr and the run goes on.  hist: per state from skip on "state c1 c2
 * ... \n"; gamma: "4\n<states>\n" and per state "state a b" with %.4f, the golden-section fit of estimate_gamma_models
 * operation for operation, "0.0000 0.0000" for a state below skip, below mincount or with fewer than two points. */
aasr_status aasr_run_dur_est(const char *ph_path, const char *recipe_path, const aasr_dur_est_options *opt);
/* estimate_gamma_models on one histogram (hist[i]: occurrences of duration i + 1).  -> 1 and *a, *b, or 0 with fewer
 * than two points.  Host only. */
int32_t aasr_dur_est_fit_gamma(const int32_t *hist, int32_t n, double *a, double *b);

/* ---- FST decoder: token passing over a compiled search network (the reference's FstSearch) ---------------------------
 * The reference's small decoder (decoder/src/FstSearch_tmpl.hh, Fst.cc, FstAcoustics.cc) restated: a frame-synchronous
 * token pass over a "#FSTBasic MaxPlus" network with state indices on the arcs, a beam, a token limit and recombination
 * on (node, word history).  One workgroup per utterance, a batch per launch (csrc/fst_search.h).  The arithmetic is
 * the reference's float operations in its order; tools/fst_restate.py is the same in NumPy and the yardstick of the tests.
 * Confidence scores (FstConfidence, FstConfidenceWithPhoneLoop): the block "FST decoder: confidence" below.
 * Out of scope: TokenPassSearch and n-grams, lattices and n-best lists, epsilon closure (the reference has none: a token
 * crosses one arc per frame), one utterance over several workgroups. */
typedef struct aasr_fstnet aasr_fstnet;
/* Fst::read (Fst.cc:10-103) with its messages in aasr_last_error() (AASR_ERR_INVALID; AASR_ERR_IO: cannot open): "Unknown
 * header", "Too few fields", "Too many fields for I:" / "F:", "Weird number of fields for T:", "Weird type indicator:",
 * "Conflicting emission_pdf_indices".  Also refused: a negative node index, no initial node.  csrc/fst_net.h. */
aasr_status aasr_fstnet_create_from_file(const char *path, aasr_fstnet **out);
void aasr_fstnet_destroy(aasr_fstnet *net);
int32_t aasr_fstnet_num_nodes(const aasr_fstnet *net);
int32_t aasr_fstnet_num_arcs(const aasr_fstnet *net);
int32_t aasr_fstnet_num_symbols(const aasr_fstnet *net);
int32_t aasr_fstnet_initial(const aasr_fstnet *net);
int32_t aasr_fstnet_max_pdf(const aasr_fstnet *net);
/* symbol `id` (ids in order of first appearance), the file's bytes; NULL outside 0 ... num_symbols - 1 */
const char *aasr_fstnet_symbol(const aasr_fstnet *net, int32_t id);
/* the CSR arrays (any may be NULL): arc_begin [nodes + 1]; arc_tgt, arc_logprob, arc_word (-1: no symbol) [arcs], file
 * order within a node; node_pdf (-1: non-emitting), node_end [nodes] */
aasr_status aasr_fstnet_arrays(const aasr_fstnet *net, int32_t *arc_begin, int32_t *arc_tgt, float *arc_logprob,
                               int32_t *arc_word, int32_t *node_pdf, int32_t *node_end);

typedef struct aasr_fst_options {
  float beam;              /* 2600; finite, >= 0                                                                      */
  int32_t token_limit;     /* 5000; the search keeps token_limit + 1 tokens, as the reference does                    */
  float duration_scale;    /* 3                                                                                        */
  float transition_scale;  /* 1                                                                                        */
  int32_t dur_by_state;    /* 0: the duration tables as the reference builds them (the file's values at [n, 2n), zeros
                              below: no duration term for pdf indices < n); 1: the file's values at [0, n)           */
  int32_t cap_candidates;  /* capacities per utterance, 0 = derived from the network and the limit: candidates per     */
  int32_t cap_recomb;      /* frame; recombination table and history table (powers of two).  Exceeding one gives the  */
  int32_t cap_history;     /* utterance an AASR_FST_OVERFLOW_* status, never a silent truncation                      */
} aasr_fst_options;
void aasr_fst_default_options(aasr_fst_options *opt);

enum {
  AASR_FST_OK = 0,
  AASR_FST_NO_TOKENS = 1,            /* no candidate at some frame (where the reference indexes an empty vector)      */
  AASR_FST_OVERFLOW_CANDIDATES = 2,
  AASR_FST_OVERFLOW_RECOMB = 3,
  AASR_FST_OVERFLOW_HISTORY = 4
};

typedef struct aasr_fst_durations aasr_fst_durations;
/* FstAcoustics::duration_read (FstAcoustics.cc:60-89): "4", the number of states, `id a b` per state.  Host only. */
aasr_status aasr_fst_durations_read(const char *path, aasr_fst_durations **out);
void aasr_fst_durations_destroy(aasr_fst_durations *dur);
int32_t aasr_fst_durations_num_states(const aasr_fst_durations *dur);
/* duration_logprob (FstAcoustics.cc:91-101) under either indexing; 0 where a <= 0 or the index is past the tables */
float aasr_fst_durations_logprob(const aasr_fst_durations *dur, int32_t dur_by_state, int32_t pdf, int32_t d);

typedef struct aasr_fst_batch aasr_fst_batch;
/* A batch of n_utt utterances of n_frames[u] >= 0 frames over one network; dur may be NULL (no duration term: + scale *
 * 0.0f).  net and dur must outlive the batch.  Needs a device. */
aasr_status aasr_fst_batch_create(const aasr_fstnet *net, const aasr_fst_durations *dur, const aasr_fst_options *opt,
                                  int32_t n_utt, const int32_t *n_frames, aasr_fst_batch **out);
void aasr_fst_batch_destroy(aasr_fst_batch *b);
int64_t aasr_fst_batch_device_bytes(const aasr_fst_batch *b);
/* the options with the derived capacities filled in (what a rerun doubles) */
void aasr_fst_batch_options(const aasr_fst_batch *b, aasr_fst_options *out);
/* The search of every utterance.  d_lna: n_rows rows of n_models values of lnabytes bytes on the device -- 2 (big-endian
 * codes) or 4 (floats) as aasr_gmm_score_lna_dev leaves them, or 1 from a file --, decoded as LnaReaderCircular does;
 * utterance u reads rows row0[u] ... row0[u] + n_frames[u] - 1.  A network whose largest pdf index is not below n_models is
 * AASR_ERR_INVALID (the reference would read out of bounds), as is a row range outside 0 ... n_rows. */
aasr_status aasr_fst_batch_dev(aasr_fst_batch *b, const void *d_lna, int32_t lnabytes, int32_t n_models, int64_t n_rows,
                               const int64_t *row0, void *stream);
/* (aasr_fst_batch_dev only queues: copies and the launch on `stream`; nothing of the caller's is read after it returns.)
 * Waits and fetches the results; n_overflow: the utterances with an AASR_FST_OVERFLOW_* status */
aasr_status aasr_fst_batch_sync(aasr_fst_batch *b, void *stream, int32_t *n_overflow);
/* Utterance u after a sync (any pointer may be NULL): status; logprob and words [n_words] of the best token at an end node
 * (none: -1.0f and no words, get_result_and_logprob); best_logprob (get_best_token_logprob, -9999999.0f without tokens);
 * best_final_logprob (-9999999.9f without an end-node token); n_tokens surviving the last frame. */
aasr_status aasr_fst_batch_result(const aasr_fst_batch *b, int32_t u, int32_t *status, float *logprob, float *best_logprob,
                                  float *best_final_logprob, int32_t *n_words, int32_t *words, int32_t cap_words,
                                  int32_t *n_tokens);
/* Every token surviving the last frame, by descending log-probability: node, logprob, dur [n_tokens], word_begin
 * [n_tokens + 1] into words (NULL: counted only).  Copies the utterance's history table from the device. */
aasr_status aasr_fst_batch_tokens(aasr_fst_batch *b, int32_t u, int32_t cap_tokens, int32_t *node, float *logprob, int32_t *dur,
                                  int32_t *word_begin, int32_t cap_words, int32_t *words);

/* ---- FST decoder: streaming sessions ------------------------------------------------------------------------------------
 * The search of aasr_fst_batch cut at feed boundaries: n_sessions live utterances whose tokens, history table and
 * counters stay on the device between launches, one launch per feed over all of them (csrc/fst_stream.h).  Whatever the
 * chunking, a session after t frames holds what aasr_fst_batch holds after an utterance of those t frames, bit for bit:
 * both kernels run one copy of the frame's arithmetic (csrc/fst_frame.h).
 * Capacities are derived as aasr_fst_batch_create derives them, with max_frames in the place of the longest utterance
 * (the same cap_* options; the duration table covers d = 0 ... max_frames; results hold max_frames + 1 words).
 * A status other than AASR_FST_OK is sticky: the session skips the frames it is fed and keeps its status, frames_done
 * and result until aasr_fst_stream_reset.  An overflow is reported and never retried behind the caller's back: a live
 * stream cannot be re-run from frames that are gone, and the tables of a live session do not grow -- choose max_frames
 * and the capacities for the longest utterance expected.  frames_done counts the frames consumed, the one that ended the
 * search (NO_TOKENS, OVERFLOW_*) included, so it does not depend on where the feeds were cut.
 * Confidence scores on a stream: aasr_fst_conf_stream_*, the block "FST decoder: confidence on streaming sessions" below.
 * Out of scope: growing a table of a live session, endpointing, one session over several workgroups.
 * One stream per handle: feeds and syncs of a handle go to the same `stream`. */
typedef struct aasr_fst_stream aasr_fst_stream;
/* Sessions start fresh.  n_sessions < 1, max_frames < 1 or a null argument: AASR_ERR_INVALID.  net and dur (may be NULL)
 * must outlive the handle.  Needs a device. */
aasr_status aasr_fst_stream_create(const aasr_fstnet *net, const aasr_fst_durations *dur, const aasr_fst_options *opt,
                                   int32_t n_sessions, int32_t max_frames, aasr_fst_stream **out);
void aasr_fst_stream_destroy(aasr_fst_stream *s);
int64_t aasr_fst_stream_device_bytes(const aasr_fst_stream *s);
/* the options with the derived capacities filled in */
void aasr_fst_stream_options(const aasr_fst_stream *s, aasr_fst_options *out);
/* Marks session u (-1: every session) fresh: the next feed starts it anew -- tables cleared, one token at the initial
 * node --, whatever its n_new.  No launch of its own; until that feed, result and tokens answer with the start state. */
aasr_status aasr_fst_stream_reset(aasr_fst_stream *s, int32_t u);
/* One feed: session u takes n_new[u] >= 0 further frames from rows row0[u] ... row0[u] + n_new[u] - 1 of d_lna (rows of
 * THIS buffer; layout and decoding as aasr_fst_batch_dev).  Only queues: a copy and one launch on `stream`; row0 and n_new
 * are not read after it returns.  A session with n_new[u] == 0 that is not fresh is left untouched.
 * Refused with AASR_ERR_INVALID before anything is queued, every session left as it was: a negative n_new[u]; frames_done +
 * n_new[u] > max_frames; a row range outside 0 ... n_rows; a network whose largest pdf index is not below n_models; an
 * lnabytes or n_models other than what a session that is not fresh was fed before.
 * frames_done is counted on the host, for the sessions whose status the last sync saw as AASR_FST_OK.  A session that went
 * sticky in a feed not yet synced is still counted (and checked against max_frames) as if it had taken its frames; the next
 * sync sets its count to the device's frames_done, and from then on its feeds are neither counted nor checked against
 * max_frames. */
aasr_status aasr_fst_stream_feed_dev(aasr_fst_stream *s, const void *d_lna, int32_t lnabytes, int32_t n_models,
                                     int64_t n_rows, const int64_t *row0, const int32_t *n_new, void *stream);
/* waits for the feeds queued on `stream` and fetches every session's record */
aasr_status aasr_fst_stream_sync(aasr_fst_stream *s, void *stream);
/* Session u after a sync (any pointer may be NULL): the fields of aasr_fst_batch_result for the frames so far, with the
 * same sentinels; frames_done; and the partial hypothesis, the words of the best token over all nodes (the token behind
 * best_logprob: the highest log-probability, the earlier token among equals -- the reference's best_tokens(1)).  A fresh
 * session that was not fed yet reports the start state (init_search()): one token, best_logprob 0.0f, no words. */
aasr_status aasr_fst_stream_result(const aasr_fst_stream *s, int32_t u, int32_t *status, int32_t *frames_done,
                                   float *logprob, float *best_logprob, float *best_final_logprob,
                                   int32_t *n_words, int32_t *words, int32_t cap_words,
                                   int32_t *n_partial_words, int32_t *partial_words, int32_t cap_partial, int32_t *n_tokens);
/* as aasr_fst_batch_tokens: the session's tokens by descending log-probability */
aasr_status aasr_fst_stream_tokens(aasr_fst_stream *s, int32_t u, int32_t cap_tokens, int32_t *node, float *logprob,
                                   int32_t *dur, int32_t *word_begin, int32_t cap_words, int32_t *words);

/* The fst_stream tool's run (csrc/fst_live.cc): headerless PCM16 (the audiofile module's byte order) from the descriptor
 * in_fd while it is still being written.  The samples are read as frames become computable (frame t when the samples
 * cover frame t + halo_r + 1, aasr_feat_halo; at the end of input the frames up to aasr_feat_eof_frame); per chunk of
 * chunk_frames frames the feature chain for exactly those frames over the samples so far, one score + LNA step
 * (aasr_gmm_score_lna_dev, normalised, lnabytes 2 or 4) and one feed of a one-session aasr_fst_stream that reads the
 * step's device buffer in place.  On stdout: with `partial`, a flushed line `frames best_logprob words...` whenever the
 * partial hypothesis differs from the one printed last; at the end of input one line `- logprob words... [STATUS]` in
 * fst_decode's format.  An input of more than max_frames frames is refused when it gets there; nothing is rerun.
 * Out of scope: speaker files, endpointing. */
typedef struct aasr_fst_live_options {
  aasr_fst_options fst;
  int32_t lnabytes;      /* 2 or 4 */
  int32_t chunk_frames;  /* 16; >= 1 */
  int32_t max_frames;    /* 7500 (one minute at 125 frames/s); >= 1 */
  int32_t partial;
  int32_t info;
  int32_t in_fd;         /* 0: standard input */
} aasr_fst_live_options;
void aasr_fst_live_default_options(aasr_fst_live_options *opt);
aasr_status aasr_run_fst_live(aasr_feat *feat, aasr_gmm *gmm, const aasr_fstnet *net, const aasr_fst_durations *dur,
                              const aasr_fst_live_options *opt, aasr_run_stats *stats);

/* fst_decode's run over a recipe (csrc/fst_decode.cc), groups of `group` utterances.  Engine mode (lna_files 0; feat and
 * gmm given): per group the recipe's audio= through the feature chain (one launch set per stretch of equal speaker
 * settings), ONE score + LNA step over the group's frames (aasr_gmm_score_lna_dev, normalised, lnabytes 2 or 4: the
 * values phone_probs would write) and one search launch that reads the step's device buffer in place -- no LNA value
 * leaves the device and no LNA file is written.  lna_files 1: the recipe's lna= files (1-, 2- or 4-byte; one width and
 * model count per group) are uploaded and searched; feat, gmm and speakers NULL.  Utterances that overflow a capacity
 * run once more with every capacity doubled (a line on stderr); those that overflow again keep their status.  Output
 * to `out` ("-": stdout), one line per utterance: the line's audio (engine mode) or lna path, the log-probability as
 * %.9g, the words, and a trailing status word (NO_TOKENS, OVERFLOW_*) when the status is not OK.  stats->seconds_device:
 * from a group's first upload to its last result, summed. */
typedef struct aasr_fst_decode_options {
  aasr_fst_options fst;
  int32_t lna_files;
  int32_t lnabytes;     /* engine mode: 2 or 4 */
  int32_t group;        /* utterances per launch, >= 1 */
  int32_t num_batches, batch_index;
  int32_t info;
  aasr_spkc *speakers;  /* engine mode: -S, or NULL */
  const char *out;
} aasr_fst_decode_options;
void aasr_fst_decode_default_options(aasr_fst_decode_options *opt);
aasr_status aasr_run_fst_decode_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_fstnet *net, const aasr_fst_durations *dur,
                                       const char *recipe_path, const aasr_fst_decode_options *opt, aasr_run_stats *stats);

/* ---- FST decoder: confidence (the reference's FstConfidence and FstConfidenceWithPhoneLoop) -----------------------------
 * A grammar search, optionally a second search over a phone-loop network on the same acoustics, the best acoustic value
 * of every frame summed per utterance, and the best surviving hypothesis whose words differ from the winner's
 * (csrc/fst_conf.h).  Neither LNA values nor token or history tables leave the device for a confidence.  All float
 * operations in the reference's order (decoder/src/FstConfidence.cc), frames an int converted to float:
 *   ploop_conf    = min(1, 1 - 0.25 * (-grammar_logprob + ploop_logprob) / frames)
 *   best_acu_conf = 1.5 - 0.25 * (-best_final_logprob + best_acu_score) / frames
 *   token_conf    = max(0, min(1, 0.2 - 5 * (-best_final_logprob + best_different_logprob) / frames)); -9999999.9f when
 *                   the best end-node token has no words
 *   edit_conf     = max(0, 1 - ldist / len): byte Levenshtein distance of the two result strings without spaces and
 *                   repeated consecutive bytes, len of the cleaned grammar string (0: IEEE division, a NaN gives 0)
 *   confidence    = (min(1, ploop) + 20 min(1, token) + 5 min(1, edit) + min(1, best_acu)) / 27
 * best_acu_score: the float sum in frame order of every frame's maximum over ALL n_models values (start -999999999.9f,
 * replaced on strict >).  best_different_logprob: the best log-probability among the surviving tokens whose word
 * sequence differs from the best end-node token's, -9999999.9f without one.
 * phone_loop 0 is the reference's plain FstConfidence: no second search, best_acu_score stays 0 (the reference computes
 * the frame maximum there and discards it; here the pass is not run), confidence = 0.5 * (token_conf + best_acu_conf)
 * (the product in double, stored to float); ploop_logprob is -1, ploop_conf and edit_conf are 0.
 * Where the reference is undefined or only noisy:
 *   no end-node token    the reference reads an uninitialised float.  Here best_final_logprob is -9999999.9f (what
 *                        get_best_final_token_logprob returns), token_conf is -9999999.9f, and no_final is set.
 *   zero frames          the IEEE result of the float division is kept.
 *   debug lines          the reference's unconditional "Ldist", "pl_lp" and "Emptiness" lines are not printed; its verbose
 *                        block goes to stderr from aasr_fst_conf_batch_result when options.verbose is not 0.
 *   unused members       the phone-loop log-probability weight, the log-probability confidence weight and hysteresis are
 *                        set and never read in the reference: they have no counterpart here (the Python classes keep
 *                        the setters). */
typedef struct aasr_fst_conf_options {
  aasr_fst_options grammar;
  aasr_fst_options phone;  /* the phone-loop search: its own beam, token limit, scales and capacities */
  int32_t phone_loop;      /* 0: FstConfidence; 1: FstConfidenceWithPhoneLoop (needs a phone-loop network) */
  int32_t verbose;
} aasr_fst_conf_options;
/* both searches 2600 / 5000 / 3 / 1, phone_loop 0, verbose 0 */
void aasr_fst_conf_default_options(aasr_fst_conf_options *opt);

typedef struct aasr_fst_conf_result {
  float confidence, token_conf, ploop_conf, edit_conf, best_acu_conf;
  float grammar_logprob, ploop_logprob, best_final_logprob, best_different_logprob, best_acu_score;
  int32_t frames;
  int32_t grammar_status, phone_status; /* AASR_FST_*; phone_status AASR_FST_OK without a phone loop */
  int32_t no_final;                     /* the grammar search left no token at an end node */
  int32_t valid;                        /* 0: a search overflowed a capacity, the floats above are 0 */
} aasr_fst_conf_result;

typedef struct aasr_fst_conf_batch aasr_fst_conf_batch;
/* One aasr_fst_batch per network (phone_net NULL without a phone loop), the frame-best and token-record buffers.  Bad
 * options (either search's), a NULL grammar and phone_loop without a network are AASR_ERR_INVALID before a device is
 * looked for.  The networks and dur must outlive the batch. */
aasr_status aasr_fst_conf_batch_create(const aasr_fstnet *grammar_net, const aasr_fstnet *phone_net, const aasr_fst_durations *dur,
                                       const aasr_fst_conf_options *opt, int32_t n_utt, const int32_t *n_frames,
                                       aasr_fst_conf_batch **out);
void aasr_fst_conf_batch_destroy(aasr_fst_conf_batch *b);
/* the options with both searches' derived capacities filled in (what a rerun doubles) */
void aasr_fst_conf_batch_options(const aasr_fst_conf_batch *b, aasr_fst_conf_options *out);
/* Queues on `stream`: the grammar search, the phone-loop search, the frame-best pass with its sums, and the token records
 * of both searches.  Arguments as aasr_fst_batch_dev; d_lna must be aligned to lnabytes. */
aasr_status aasr_fst_conf_batch_dev(aasr_fst_conf_batch *b, const void *d_lna, int32_t lnabytes, int32_t n_models, int64_t n_rows,
                                    const int64_t *row0, void *stream);
/* the frame-best pass and its sums alone (what aasr_fst_conf_batch_dev queues for them); also without a phone loop */
aasr_status aasr_fst_conf_batch_frame_best_dev(aasr_fst_conf_batch *b, const void *d_lna, int32_t lnabytes, int32_t n_models,
                                               int64_t n_rows, const int64_t *row0, void *stream);
/* Waits, fetches the per-utterance records and both searches' results, and computes the confidences on the host */
aasr_status aasr_fst_conf_batch_sync(aasr_fst_conf_batch *b, void *stream, int32_t *n_overflow);
aasr_status aasr_fst_conf_batch_result(const aasr_fst_conf_batch *b, int32_t u, aasr_fst_conf_result *out);
/* the inner batches, for aasr_fst_batch_result and aasr_fst_batch_tokens; phone: NULL without a phone loop */
aasr_fst_batch *aasr_fst_conf_batch_grammar(aasr_fst_conf_batch *b);
aasr_fst_batch *aasr_fst_conf_batch_phone(aasr_fst_conf_batch *b);
/* The device's record of utterance u for the grammar search (phone 0) or the phone-loop search (phone 1), after a sync:
 * whether a token stands at an end node, the words of the best such token, whether a token with other words survives,
 * and the two log-probabilities (-9999999.9f where there is none).  Any pointer may be NULL. */
aasr_status aasr_fst_conf_batch_record(const aasr_fst_conf_batch *b, int32_t u, int32_t phone, int32_t *has_final, int32_t *n_words,
                                       int32_t *has_different, float *best_final_logprob, float *best_different_logprob);
/* the frame-best values of utterance u [n_frames[u]] and their sum, copied from the device after a frame-best pass */
aasr_status aasr_fst_conf_batch_frame_best(aasr_fst_conf_batch *b, int32_t u, void *stream, float *best, int32_t cap, float *sum);
/* The host's part alone (no device): the cleaned string of remove_junk into out (cap bytes, -> its length or -1), the
 * byte edit distance, and the formulas on given inputs (grammar, ploop: the result strings, ploop NULL: plain). */
int32_t aasr_fst_conf_remove_junk(const char *s, int32_t n, char *out, int32_t cap);
int32_t aasr_fst_conf_edit_distance(const char *a, int32_t na, const char *b, int32_t nb);
void aasr_fst_conf_formulas(aasr_fst_conf_result *r, int32_t n_words, const char *grammar, int32_t n_grammar, const char *ploop,
                            int32_t n_ploop);

/* ---- FST decoder: confidence on streaming sessions ---------------------------------------------------------------------
 * aasr_fst_conf_batch cut at feed boundaries: n_sessions live utterances whose two searches (aasr_fst_stream's state, once
 * per network), token records and best-acoustics sums stay on the device between launches.  One launch per feed runs a
 * session's grammar search, its phone-loop search and its sum as sibling workgroups (csrc/fst_conf_stream.h), so a feed
 * waits for the slower of the two searches, not for one after the other.
 * The contract: after any sequence of feeds that gave a session t frames since its reset, aasr_fst_conf_stream_result is
 * field for field and bit for bit what aasr_fst_conf_batch returns for an utterance of those t rows under the same options
 * -- t = 0 with its IEEE division; AASR_FST_NO_TOKENS in either search (valid, the sentinels as in the batch);
 * AASR_FST_OVERFLOW_* in either search (valid 0, floats 0, the statuses reported).  A confidence is there at every feed
 * boundary, not only at the end.
 * Capacities: as aasr_fst_stream_create derives them, for both searches, with max_frames in the place of the longest
 * utterance; the phone loop's derived history table is the confidence batch's larger one.
 * Each search's status is sticky as in aasr_fst_stream and an overflow is never rerun.  The sum is carried for every fed
 * frame whatever the searches' statuses, and so is `frames`: this handle counts the frames fed per session for every
 * accepted feed; each search's own frames_done is reported by aasr_fst_conf_stream_search_result.
 * One stream per handle: feeds and syncs of a handle go to the same `stream`. */
typedef struct aasr_fst_conf_stream aasr_fst_conf_stream;
/* Sessions start fresh.  phone_net NULL without a phone loop.  A null argument, n_sessions < 1, max_frames < 1, bad options
 * of either search and phone_loop without a network are AASR_ERR_INVALID before a device is looked for.  The networks and
 * dur (may be NULL) must outlive the handle. */
aasr_status aasr_fst_conf_stream_create(const aasr_fstnet *grammar_net, const aasr_fstnet *phone_net, const aasr_fst_durations *dur,
                                        const aasr_fst_conf_options *opt, int32_t n_sessions, int32_t max_frames,
                                        aasr_fst_conf_stream **out);
void aasr_fst_conf_stream_destroy(aasr_fst_conf_stream *s);
int64_t aasr_fst_conf_stream_device_bytes(const aasr_fst_conf_stream *s);
/* the options with both searches' derived capacities filled in */
void aasr_fst_conf_stream_options(const aasr_fst_conf_stream *s, aasr_fst_conf_options *out);
/* Marks session u (-1: every session) fresh, as aasr_fst_stream_reset: both searches and the sum start anew at the next
 * feed; until then the session answers with the zero-frame result of the batch. */
aasr_status aasr_fst_conf_stream_reset(aasr_fst_conf_stream *s, int32_t u);
/* One feed, arguments as aasr_fst_stream_feed_dev.  Only queues: one small copy and the one launch on `stream`.  Refused
 * with AASR_ERR_INVALID before anything is queued, every session left as it was: a negative n_new[u]; frames fed + n_new[u]
 * > max_frames; a row range outside 0 ... n_rows; a pdf of either network that is not below n_models; an lnabytes or
 * n_models other than what a session that is not fresh was fed before; d_lna not aligned to lnabytes. */
aasr_status aasr_fst_conf_stream_feed_dev(aasr_fst_conf_stream *s, const void *d_lna, int32_t lnabytes, int32_t n_models, int64_t n_rows,
                                          const int64_t *row0, const int32_t *n_new, void *stream);
/* Waits for the feeds queued on `stream`, fetches the records, the sums and both searches' results, and computes the
 * confidences on the host with aasr_fst_conf_batch_sync's own code. */
aasr_status aasr_fst_conf_stream_sync(aasr_fst_conf_stream *s, void *stream);
/* session u after a sync: the fields of aasr_fst_conf_batch_result for the frames fed so far */
aasr_status aasr_fst_conf_stream_result(const aasr_fst_conf_stream *s, int32_t u, aasr_fst_conf_result *out);
/* The grammar search (phone 0) or the phone-loop search (phone 1) of session u: as aasr_fst_stream_result and
 * aasr_fst_stream_tokens.  phone 1 without a phone loop is AASR_ERR_INVALID. */
aasr_status aasr_fst_conf_stream_search_result(const aasr_fst_conf_stream *s, int32_t u, int32_t phone, int32_t *status,
                                               int32_t *frames_done, float *logprob, float *best_logprob, float *best_final_logprob,
                                               int32_t *n_words, int32_t *words, int32_t cap_words, int32_t *n_partial_words,
                                               int32_t *partial_words, int32_t cap_partial, int32_t *n_tokens);
aasr_status aasr_fst_conf_stream_tokens(aasr_fst_conf_stream *s, int32_t u, int32_t phone, int32_t cap_tokens, int32_t *node,
                                        float *logprob, int32_t *dur, int32_t *word_begin, int32_t cap_words, int32_t *words);
/* the device's token record of session u, as aasr_fst_conf_batch_record */
aasr_status aasr_fst_conf_stream_record(const aasr_fst_conf_stream *s, int32_t u, int32_t phone, int32_t *has_final, int32_t *n_words,
                                        int32_t *has_different, float *best_final_logprob, float *best_different_logprob);
/* the carried sum of the frames' best acoustic values and the frames it covers (with a phone loop only: the plain
 * FstConfidence never uses the sum, and it is not carried) */
aasr_status aasr_fst_conf_stream_best_acu(const aasr_fst_conf_stream *s, int32_t u, float *sum, int32_t *frames);

/* fst_stream --confidence (csrc/fst_live.cc): aasr_run_fst_live's chunk loop with a one-session aasr_fst_conf_stream in
 * the place of the aasr_fst_stream.  With live.partial the lines are `frames best_logprob confidence words...`; the final
 * line is fst_decode --confidence's with `-` as the path: `- logprob confidence words... [STATUS]` (the grammar's status
 * first, else the phone loop's). */
typedef struct aasr_fst_live_confidence_options {
  aasr_fst_live_options live;  /* live.fst is the grammar search */
  aasr_fst_options phone;
  int32_t phone_loop;
} aasr_fst_live_confidence_options;
void aasr_fst_live_confidence_default_options(aasr_fst_live_confidence_options *opt);
aasr_status aasr_run_fst_live_confidence(aasr_feat *feat, aasr_gmm *gmm, const aasr_fstnet *net, const aasr_fstnet *phone_net,
                                         const aasr_fst_durations *dur, const aasr_fst_live_confidence_options *opt,
                                         aasr_run_stats *stats);

/* fst_decode --confidence over a recipe: the group loop of aasr_run_fst_decode_recipe with a confidence batch per group;
 * the group's LNA device buffer feeds both searches and the frame-best pass.  Output lines: path, log-probability and
 * confidence as %.9g, the words, and a trailing status word when a search's status is not OK (the grammar's first). */
typedef struct aasr_fst_confidence_options {
  aasr_fst_decode_options decode;  /* decode.fst is the grammar search */
  aasr_fst_options phone;
  int32_t phone_loop;
} aasr_fst_confidence_options;
void aasr_fst_confidence_default_options(aasr_fst_confidence_options *opt);
aasr_status aasr_run_fst_confidence_recipe(aasr_feat *feat, aasr_gmm *gmm, const aasr_fstnet *net, const aasr_fstnet *phone_net,
                                           const aasr_fst_durations *dur, const char *recipe_path,
                                           const aasr_fst_confidence_options *opt, aasr_run_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* AASR_H */
