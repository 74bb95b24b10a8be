"""capi.py -- ctypes binding of libaasr.so (the C ABI in include/aasr.h).

The Python binding of the engine: every function of include/aasr.h with its argument types, plus
thin handle classes (Feat, Gmm, SpeakerConfig) that mirror aku::FeatureGenerator / HmmSet /
SpeakerConfig call for call.  Tests, bench.py and the pipeline / shard helpers go through it; it
holds no arithmetic of its own.  It never falls back to a CPU path: if the shared library is
missing it raises, and compute calls without a HIP device return AASR_ERR_NO_DEVICE.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# AASR_LIBDIR: another build of the same library (the ablation build of tools/, aaltoasr_amd/lib_ablation)
LIB_PATH = os.path.join(os.environ.get("AASR_LIBDIR") or os.path.join(HERE, "lib"), "libaasr.so")
HEADER_PATH = os.path.join(HERE, "..", "include", "aasr.h")

AASR_OK = 0
AASR_ERR_INVALID = -1
AASR_ERR_UNSUPPORTED = -2
AASR_ERR_NO_DEVICE = -3
AASR_ERR_IO = -4
AASR_ERR_SHORT_AUDIO = -5


class AasrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("aasr status %d: %s" % (code, msg))
        self.code = code
        self.msg = msg


class RunOptions(C.Structure):
    _fields_ = [("lnabytes", C.c_int32), ("normalize", C.c_int32), ("num_batches", C.c_int32),
                ("batch_index", C.c_int32), ("no_overwrite", C.c_int32), ("raw_audio", C.c_int32),
                ("info", C.c_int32), ("afname", C.c_int32), ("out_dir", C.c_char_p),
                ("speakers", C.c_void_p), ("sort_recipe", C.c_int32)]


class RunStats(C.Structure):
    _fields_ = [("utterances", C.c_int64), ("frames", C.c_int64),
                ("seconds_total", C.c_double), ("seconds_device", C.c_double),
                ("seconds_copy_out", C.c_double)]


class RecipeTiming(C.Structure):
    _fields_ = [("seconds_total", C.c_double), ("wait_reader", C.c_double), ("wait_result_slot", C.c_double),
                ("enqueue", C.c_double), ("wait_copies", C.c_double), ("device", C.c_double),
                ("copy_out", C.c_double), ("writer_threads", C.c_int32), ("usable_cores", C.c_int32),
                ("host_share", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: (round(getattr(self, k), 4) if t is C.c_double else int(getattr(self, k))) for k, t in self._fields_}


_lib: Optional[C.CDLL] = None
# aasr_tie_gain_fn: (user, n_members, members, n_set, set) -> gain
TIE_GAIN_FN = C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32))


def declared_symbols() -> list:
    """Function names declared in include/aasr.h."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(aasr_[a-z0-9_]+)\s*\(", text)))


def lib() -> C.CDLL:
    """Loads libaasr.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libaasr.so is missing (%s): build it with `python -m aaltoasr_amd.build`; "
            "this engine has no CPU fallback" % LIB_PATH)
    # torch bundles its own libamdhip64.so.7; importing it first makes both
    # share one HIP runtime so torch device pointers are valid in libaasr.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    _declare(L)
    _lib = L
    return L


def _declare(L: C.CDLL) -> None:
    i32, i64, f, d, vp, cp = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_void_p, C.c_char_p
    pvp = C.POINTER(vp)
    L.aasr_last_error.restype = cp
    # forced alignment
    L.aasr_topo_create_from_ph.argtypes = [cp, pvp]
    L.aasr_topo_destroy.argtypes = [vp]
    L.aasr_topo_destroy.restype = None
    L.aasr_topo_num_hmms.argtypes = [vp]
    L.aasr_topo_hmm_index.argtypes = [vp, cp]
    L.aasr_topo_hmm_label.argtypes = [vp, i32]
    L.aasr_topo_hmm_label.restype = cp
    L.aasr_topo_hmm_num_states.argtypes = [vp, i32]
    L.aasr_topo_hmm_states.argtypes = [vp, i32, vp]
    L.aasr_topo_num_states.argtypes = [vp]
    L.aasr_topo_state_num_transitions.argtypes = [vp, i32]
    L.aasr_topo_state_transitions.argtypes = [vp, i32, vp, vp]
    L.aasr_topo_max_offset.argtypes = [vp]
    L.aasr_topo_validate.argtypes = [vp, vp]
    L.aasr_topo_check_states.argtypes = [vp, i32]
    L.aasr_align_default_options.argtypes = [vp]
    L.aasr_align_default_options.restype = None
    L.aasr_align_read_transcript.argtypes = [vp, cp, f, i32, i32, C.POINTER(C.POINTER(i32)), C.POINTER(i32)]
    L.aasr_align_format_line.argtypes = [f, i32, i32, cp, cp, cp, i32]
    L.aasr_align_batch_create.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, pvp]
    L.aasr_align_batch_destroy.argtypes = [vp]
    L.aasr_align_batch_destroy.restype = None
    L.aasr_align_batch_rows.argtypes = [vp, i32]
    L.aasr_align_batch_device_bytes.argtypes = [vp]
    L.aasr_align_batch_device_bytes.restype = i64
    L.aasr_align_batch_dev.argtypes = [vp, vp, vp, i64, i32, vp, i32, vp]
    L.aasr_align_batch_sync.argtypes = [vp, vp, C.POINTER(i32)]
    L.aasr_align_batch_result.argtypes = [vp, i32, vp, C.POINTER(i32), C.POINTER(d), C.POINTER(i32), C.POINTER(i32)]
    L.aasr_run_align_recipe.argtypes = [vp, vp, vp, cp, vp, vp]
    # ML statistics
    L.aasr_feat_run_f64_dev.argtypes = [vp, vp, i64, i32, i32, vp, vp]
    L.aasr_stats_read_segmentation.argtypes = [vp, cp, f, i32, i32, i32, i32, C.POINTER(i32),
                                               C.POINTER(C.POINTER(i32)), C.POINTER(C.POINTER(i32)), C.POINTER(i32)]
    L.aasr_stats_write_gks.argtypes = [cp, i32, i32, i32, vp, vp, vp, vp, vp]
    L.aasr_stats_write_mcs.argtypes = [cp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.aasr_stats_write_phs.argtypes = [cp, i32, vp, vp, vp]
    L.aasr_stats_write_lls.argtypes = [cp, d, i64]
    L.aasr_stats_create.argtypes = [vp, vp, pvp]
    L.aasr_stats_create_full.argtypes = [vp, vp, pvp]
    L.aasr_stats_mode.argtypes = [vp]
    L.aasr_stats_mode.restype = i32
    L.aasr_stats_full_moments.argtypes = [vp, vp]
    L.aasr_stats_write_gks_full.argtypes = [cp, i32, i32, vp, vp, vp, vp, vp]
    L.aasr_debug_stats_full_shape.argtypes = [vp, C.POINTER(i32)]
    L.aasr_debug_stats_full_shape.restype = None
    L.aasr_debug_stats_set_slab_bytes.argtypes = [vp, i64]
    L.aasr_stats_destroy.argtypes = [vp]
    L.aasr_stats_destroy.restype = None
    L.aasr_stats_accumulate_dev.argtypes = [vp, vp, i64, vp, vp, vp]
    L.aasr_stats_accumulate_weighted_dev.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    L.aasr_stats_add_transitions.argtypes = [vp, vp, i64]
    L.aasr_stats_fetch.argtypes = [vp, vp]
    L.aasr_stats_gaussians.argtypes = [vp, vp, vp, vp, vp, vp]
    L.aasr_stats_mixtures.argtypes = [vp, vp, vp, vp]
    L.aasr_stats_num_transitions.argtypes = [vp]
    L.aasr_stats_transitions.argtypes = [vp, vp, vp, vp]
    L.aasr_stats_write.argtypes = [vp, cp]
    L.aasr_stats_default_options.argtypes = [vp]
    L.aasr_stats_default_options.restype = None
    L.aasr_run_stats_recipe.argtypes = [vp, vp, vp, cp, vp, vp]
    L.aasr_stats_network_default_options.argtypes = [vp]
    L.aasr_stats_network_default_options.restype = None
    L.aasr_run_stats_networks_recipe.argtypes = [vp, vp, vp, cp, vp, vp, vp]
    L.aasr_segll_create.argtypes = [vp, pvp]
    L.aasr_segll_destroy.argtypes = [vp]
    L.aasr_segll_destroy.restype = None
    L.aasr_segll_score_dev.argtypes = [vp, vp, i64, vp, vp, vp]
    L.aasr_debug_segll_shape.argtypes = [vp, C.POINTER(i32)]
    L.aasr_debug_segll_shape.restype = None
    L.aasr_phn_read_segmentation.argtypes = [vp, cp, f, i32, i32, i32, i32, i32, C.POINTER(i32),
                                             C.POINTER(C.POINTER(i32)), C.POINTER(C.POINTER(i32)), C.POINTER(i32)]
    # HMM networks and the forward-backward pass
    L.aasr_hmmnet_read.argtypes = [vp, cp, pvp]
    L.aasr_hmmnet_destroy.argtypes = [vp]
    L.aasr_hmmnet_destroy.restype = None
    L.aasr_hmmnet_counts.argtypes = [vp, vp]
    L.aasr_hmmnet_array.argtypes = [vp, i32, vp, i64, C.POINTER(i64)]
    L.aasr_hmmnet_arc_label.argtypes = [vp, i32]
    L.aasr_hmmnet_arc_label.restype = cp
    L.aasr_fb_default_options.argtypes = [vp]
    L.aasr_fb_default_options.restype = None
    L.aasr_fb_batch_create.argtypes = [vp, i32, vp, vp, pvp]
    L.aasr_fb_batch_destroy.argtypes = [vp]
    L.aasr_fb_batch_destroy.restype = None
    L.aasr_fb_batch_device_bytes.argtypes = [vp]
    L.aasr_fb_batch_device_bytes.restype = i64
    L.aasr_fb_batch_dev.argtypes = [vp, vp, i64, i64, i32, vp, i32, vp]
    L.aasr_fb_batch_sync.argtypes = [vp, vp, C.POINTER(i32)]
    L.aasr_fb_batch_result.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(d), C.POINTER(d), C.POINTER(i32), vp, vp]
    L.aasr_debug_fb_shape.argtypes = [vp, C.POINTER(i32)]
    L.aasr_debug_fb_shape.restype = None
    L.aasr_fb_batch_entries_dev.argtypes = [vp, i32, vp, vp, vp, pvp, pvp]
    L.aasr_fb_batch_entries_host.argtypes = [vp, vp, vp]
    L.aasr_fb_batch_frame_sums.argtypes = [vp, i32, vp]
    L.aasr_fb_batch_path.argtypes = [vp, i32, vp]
    L.aasr_dur_est_default_options.argtypes = [vp]
    L.aasr_dur_est_default_options.restype = None
    L.aasr_run_dur_est.argtypes = [cp, cp, vp]
    L.aasr_dur_est_fit_gamma.argtypes = [vp, i32, C.POINTER(d), C.POINTER(d)]
    L.aasr_debug_fb_entries_shape.argtypes = [vp, C.POINTER(i32)]
    L.aasr_debug_fb_entries_shape.restype = None
    L.aasr_fb_batch_frame_entries_dev.argtypes = [vp, i32, vp, i64, vp, C.POINTER(i64), pvp, pvp, pvp]
    L.aasr_fb_batch_frame_entries_host.argtypes = [vp, vp, vp, vp]
    L.aasr_debug_fb_frame_entries_shape.argtypes = [vp, C.POINTER(i32)]
    L.aasr_debug_fb_frame_entries_shape.restype = None
    L.aasr_logl_default_options.argtypes = [vp]
    L.aasr_logl_default_options.restype = None
    L.aasr_run_logl_recipe.argtypes = [vp, vp, vp, cp, vp, C.POINTER(d), vp]
    L.aasr_vtln_default_options.argtypes = [vp]
    L.aasr_vtln_default_options.restype = None
    L.aasr_vtln_grid.argtypes = [vp, C.POINTER(f), C.POINTER(f), C.POINTER(i32)]
    L.aasr_vtln_grid.restype = None
    L.aasr_vtln_summary_text.argtypes = [C.POINTER(cp), i32, vp, vp, vp, C.POINTER(vp), C.POINTER(i64)]
    L.aasr_debug_vtln_set_group_frames.argtypes = [i64]
    L.aasr_debug_vtln_set_group_frames.restype = None
    L.aasr_run_vtln_recipe.argtypes = [vp, vp, vp, cp, vp, vp]
    # CMLLR estimation
    L.aasr_mllr_create.argtypes = [vp, pvp]
    L.aasr_mllr_destroy.argtypes = [vp]
    L.aasr_mllr_destroy.restype = None
    L.aasr_mllr_reset.argtypes = [vp, vp]
    L.aasr_mllr_accumulate_dev.argtypes = [vp, vp, i64, vp, vp]
    L.aasr_mllr_accumulate_weighted_dev.argtypes = [vp, vp, i64, vp, vp, vp, i64, vp]
    L.aasr_mllr_network_default_options.argtypes = [vp]
    L.aasr_mllr_network_default_options.restype = None
    L.aasr_run_mllr_networks_recipe.argtypes = [vp, vp, vp, cp, vp, vp, vp]
    L.aasr_mllr_fetch.argtypes = [vp, vp]
    L.aasr_mllr_get.argtypes = [vp, vp, vp, C.POINTER(d)]
    L.aasr_mllr_solve.argtypes = [i32, vp, vp, d, vp]
    L.aasr_mllr_compose.argtypes = [i32, vp, vp, vp, vp, vp]
    L.aasr_mllr_default_options.argtypes = [vp]
    L.aasr_mllr_default_options.restype = None
    L.aasr_run_mllr_recipe.argtypes = [vp, vp, vp, cp, vp, vp]
    L.aasr_scatter_create.argtypes = [i32, i32, pvp]
    L.aasr_scatter_destroy.argtypes = [vp]
    L.aasr_scatter_destroy.restype = None
    L.aasr_scatter_accumulate_dev.argtypes = [vp, vp, i64, vp, vp, vp]
    L.aasr_scatter_accumulate_weighted_dev.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    L.aasr_scatter_fetch.argtypes = [vp, vp]
    L.aasr_scatter_get.argtypes = [vp, vp, vp, vp]
    L.aasr_debug_scatter_shape.argtypes = [vp, vp]
    L.aasr_debug_scatter_shape.restype = None
    L.aasr_debug_scatter_set_slab_bytes.argtypes = [vp, i64]
    L.aasr_lda_solve.argtypes = [i32, i32, vp, vp, vp, vp, d, i32, vp]
    L.aasr_lda_select.argtypes = [i32, vp, d, i32, i32, vp, i32, vp]
    L.aasr_lda_default_options.argtypes = [vp]
    L.aasr_lda_default_options.restype = None
    L.aasr_run_lda_recipe.argtypes = [cp, vp, cp, vp, vp]
    L.aasr_lda_network_default_options.argtypes = [vp]
    L.aasr_lda_network_default_options.restype = None
    L.aasr_lda_networks_check.argtypes = [cp, vp, cp, vp]
    L.aasr_run_lda_networks_recipe.argtypes = [cp, vp, vp, cp, vp, vp, vp]
    # Gaussian-pool clustering
    L.aasr_gcluster_assign.argtypes = [i32, i32, vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp]
    L.aasr_gcluster_centres.argtypes = [i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]
    L.aasr_debug_gcluster_chunk.argtypes = []
    L.aasr_debug_gcluster_chunk.restype = i32
    L.aasr_gcluster_default_options.argtypes = [vp]
    L.aasr_gcluster_default_options.restype = None
    L.aasr_run_gcluster.argtypes = [cp, cp, vp]
    L.aasr_gcluster_arrays.argtypes = [i32, i32, vp, vp, vp, vp]
    L.aasr_gmm_cluster.argtypes = [vp, i32, i32]
    # feature normalization and PCA
    L.aasr_moments_create.argtypes = [i32, i32, pvp]
    L.aasr_moments_destroy.argtypes = [vp]
    L.aasr_moments_destroy.restype = None
    L.aasr_moments_accumulate_dev.argtypes = [vp, vp, i64, vp, i32, vp]
    L.aasr_moments_fetch.argtypes = [vp, vp]
    L.aasr_moments_num_segments.argtypes = [vp]
    L.aasr_moments_num_segments.restype = i64
    L.aasr_moments_get.argtypes = [vp, vp, vp, vp, vp]
    L.aasr_moments_blocked.argtypes = [vp, i32, vp, vp, vp, vp]
    L.aasr_debug_moments_shape.argtypes = [vp, vp]
    L.aasr_debug_moments_shape.restype = None
    L.aasr_debug_moments_set_launch_segments.argtypes = [vp, i32]
    L.aasr_feanorm_pca.argtypes = [i32, vp, vp, i32, vp, vp]
    L.aasr_feanorm_default_options.argtypes = [vp]
    L.aasr_feanorm_default_options.restype = None
    L.aasr_run_feanorm_recipe.argtypes = [cp, cp, vp, vp]
    L.aasr_estimate_create.argtypes = [cp, cp, cp, pvp]
    L.aasr_estimate_destroy.argtypes = [vp]
    L.aasr_estimate_destroy.restype = None
    L.aasr_estimate_add_dump.argtypes = [vp, cp, i32]
    L.aasr_estimate_set_gaussian_parameters.argtypes = [vp, d, d]
    L.aasr_estimate_transitions.argtypes = [vp]
    L.aasr_estimate_ml.argtypes = [vp, i32, i32]
    L.aasr_estimate_delete_gaussians.argtypes = [vp, d, vp, vp]
    L.aasr_estimate_remove_mixture_components.argtypes = [vp, d, vp, vp]
    L.aasr_estimate_split_gaussians.argtypes = [vp, d, i32, i32, d, vp]
    L.aasr_estimate_write_gk.argtypes = [vp, cp]
    L.aasr_estimate_write_mc.argtypes = [vp, cp]
    L.aasr_estimate_write_ph.argtypes = [vp, cp]
    L.aasr_estimate_sizes.argtypes = [vp, vp]
    L.aasr_estimate_sizes.restype = None
    L.aasr_estimate_get_statistics.argtypes = [vp, vp, vp, vp, vp, vp]
    L.aasr_estimate_get_mixture_statistics.argtypes = [vp, vp, vp, vp]
    L.aasr_estimate_get_transition_statistics.argtypes = [vp, vp, vp]
    L.aasr_estimate_get_gaussians.argtypes = [vp, vp, vp]
    L.aasr_estimate_get_mixtures.argtypes = [vp, vp, vp, vp]
    L.aasr_estimate_get_transitions.argtypes = [vp, vp, vp, vp]
    L.aasr_mllt_create.argtypes = [i32, i64, vp, vp, vp, vp, pvp]
    L.aasr_mllt_destroy.argtypes = [vp]
    L.aasr_mllt_destroy.restype = None
    L.aasr_mllt_get_covariances.argtypes = [vp, vp]
    L.aasr_mllt_variances.argtypes = [vp, vp, vp]
    L.aasr_mllt_g_sums.argtypes = [vp, vp, vp]
    L.aasr_mllt_update_rows.argtypes = [i32, vp, d, i32, vp]
    L.aasr_mllt_estimate.argtypes = [vp, d, vp, vp, vp]
    L.aasr_debug_mllt_shape.argtypes = [vp, vp]
    L.aasr_debug_mllt_shape.restype = None
    L.aasr_debug_mllt_times.argtypes = [vp, vp]
    L.aasr_debug_mllt_times.restype = None
    L.aasr_debug_mllt_set_slab_bytes.argtypes = [vp, i64]
    L.aasr_estimate_run_mllt.argtypes = [vp, vp, vp, vp]
    L.aasr_estimate_default_options.argtypes = [vp]
    L.aasr_estimate_default_options.restype = None
    L.aasr_run_estimate.argtypes = [vp]
    # state tying
    ptext = [C.POINTER(vp), C.POINTER(i64)]
    L.aasr_tie_parse_label.argtypes = [cp] + ptext
    L.aasr_tie_create.argtypes = [i32, cp, pvp]
    L.aasr_tie_destroy.argtypes = [vp]
    L.aasr_tie_destroy.restype = None
    L.aasr_tie_num_rules.argtypes = [vp]
    L.aasr_tie_num_classes.argtypes = [vp]
    L.aasr_tie_rules_text.argtypes = [vp] + ptext
    L.aasr_tie_context_phone.argtypes = [vp, cp, i32, C.POINTER(i32)]
    L.aasr_tie_set_stats.argtypes = [vp, vp, vp, vp]
    L.aasr_tie_evaluate.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, vp, vp]
    L.aasr_tie_split.argtypes = [vp, i32, d, i32, i32, i32]
    L.aasr_tie_merge.argtypes = [vp, d, i32]
    L.aasr_tie_clusters_text.argtypes = [vp] + ptext
    L.aasr_tie_basebind_text.argtypes = [vp, i32] + ptext
    L.aasr_tie_write_basebind.argtypes = [vp, cp, i32]
    L.aasr_tie_write_model.argtypes = [vp, cp, i32]
    L.aasr_debug_tie_set_occupancy.argtypes = [vp, vp]
    L.aasr_debug_tie_split_given.argtypes = [vp, i32, d, i32, TIE_GAIN_FN, vp]
    L.aasr_debug_tie_shape.argtypes = [vp, vp]
    L.aasr_debug_tie_shape.restype = None
    L.aasr_tie_default_options.argtypes = [vp]
    L.aasr_tie_default_options.restype = None
    L.aasr_run_tie_recipe.argtypes = [cp, cp, vp, vp]
    L.aasr_spkc_write_text.argtypes = [vp, vp, i32, vp, i32, C.POINTER(vp), C.POINTER(i64)]
    L.aasr_version.restype = cp
    L.aasr_device_count.restype = C.c_int
    L.aasr_set_device.argtypes = [C.c_int]
    L.aasr_feat_create.argtypes = [cp, pvp]
    L.aasr_feat_destroy.argtypes = [vp]
    L.aasr_feat_destroy.restype = None
    L.aasr_feat_dim.argtypes = [vp]
    L.aasr_feat_frame_rate.argtypes = [vp]
    L.aasr_feat_frame_rate.restype = f
    L.aasr_feat_sample_rate.argtypes = [vp]
    L.aasr_feat_module_dim.argtypes = [vp, cp]
    L.aasr_feat_halo.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.aasr_feat_halo.restype = None
    L.aasr_feat_last_frame.argtypes = [vp, i64]
    L.aasr_feat_eof_frame.argtypes = [vp, i64]
    L.aasr_feat_run.argtypes = [vp, vp, i64, i32, i32, cp, vp]
    L.aasr_feat_run_dev.argtypes = [vp, vp, i64, i32, i32, vp, vp]
    L.aasr_feat_run_f64.argtypes = [vp, vp, i64, i32, i32, cp, vp]
    L.aasr_feat_run_batch_dev.argtypes = [vp, vp, vp, vp, i32, vp, vp]
    L.aasr_feat_set_parameters.argtypes = [vp, cp, cp]
    L.aasr_feat_run_features.argtypes = [vp, vp, i64, i32, i32, cp, vp]
    L.aasr_feat_run_features_f64.argtypes = [vp, vp, i64, i32, i32, cp, vp]
    L.aasr_feat_input_is_features.argtypes = [vp]
    L.aasr_feat_pre_legacy.argtypes = [vp]
    L.aasr_feat_input_dim.argtypes = [vp]
    L.aasr_gmm_create_diag.argtypes = [i32, i32, vp, vp, i32, vp, vp, vp, pvp]
    L.aasr_gmm_create_full.argtypes = [i32, i32, vp, vp, i32, vp, vp, vp, pvp]
    L.aasr_gmm_create_from_files.argtypes = [cp, cp, cp, pvp]
    L.aasr_gmm_destroy.argtypes = [vp]
    L.aasr_gmm_destroy.restype = None
    L.aasr_gmm_dim.argtypes = [vp]
    L.aasr_gmm_num_states.argtypes = [vp]
    L.aasr_gmm_num_gaussians.argtypes = [vp]
    L.aasr_gmm_expanded_rows.argtypes = [vp]
    L.aasr_gmm_expanded_rows.restype = i64
    L.aasr_gmm_write_cache.argtypes = [vp, cp]
    L.aasr_gmm_create_from_cache.argtypes = [cp, C.POINTER(vp)]
    L.aasr_gmm_score_scratch_floats.argtypes = [vp, i64]
    L.aasr_gmm_score_scratch_floats.restype = i64
    L.aasr_gmm_score_lna_dev.argtypes = [vp, vp, i64, C.c_int, C.c_int, vp, vp, vp]
    L.aasr_gmm_create_from_cache_checked.argtypes = [cp, cp, cp, cp, C.POINTER(vp)]
    L.aasr_recipe_frame_limits.argtypes = [C.c_float, C.c_float, C.c_float, C.POINTER(i32), C.POINTER(i32)]
    L.aasr_recipe_frame_limits.restype = None
    L.aasr_gmm_set_precision.argtypes = [vp, C.c_int]
    L.aasr_gmm_set_cmllr.argtypes = [vp, i32, vp, vp]
    L.aasr_gmm_read_clustering.argtypes = [vp, cp]
    L.aasr_gmm_set_clustering.argtypes = [vp, i32, i64, vp, vp]
    L.aasr_gmm_set_clustering_min_evals.argtypes = [vp, C.c_double, C.c_double]
    L.aasr_gmm_num_clusters.argtypes = [vp]
    L.aasr_gmm_num_clusters.restype = i32
    L.aasr_gmm_score.argtypes = [vp, vp, i64, vp]
    L.aasr_gmm_score_dev.argtypes = [vp, vp, i64, vp, vp]
    L.aasr_gmm_gauss_loglik.argtypes = [vp, vp, i64, vp]
    L.aasr_gmm_gauss_loglik_dev.argtypes = [vp, vp, i64, vp, vp]
    L.aasr_lna_encode.argtypes = [vp, i64, i32, C.c_int, C.c_int, vp, vp]
    L.aasr_lna_encode_dev.argtypes = [vp, i64, i32, C.c_int, C.c_int, vp, vp, vp]
    L.aasr_lna_header.argtypes = [i32, C.c_int, vp]
    L.aasr_lna_header.restype = None
    L.aasr_spkc_create.argtypes = [vp, vp, C.POINTER(vp)]
    L.aasr_spkc_destroy.argtypes = [vp]
    L.aasr_spkc_destroy.restype = None
    L.aasr_spkc_set_model.argtypes = [vp, vp]
    L.aasr_spkc_read_file.argtypes = [vp, cp]
    L.aasr_spkc_read_text.argtypes = [vp, cp]
    L.aasr_spkc_set_speaker.argtypes = [vp, cp]
    L.aasr_spkc_set_utterance.argtypes = [vp, cp]
    L.aasr_spkc_num_changes.argtypes = [vp]
    L.aasr_spkc_num_changes.restype = i64
    L.aasr_recipe_batch_range.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.aasr_run_recipe.argtypes = [vp, vp, cp, C.POINTER(RunOptions), C.POINTER(RunStats)]
    L.aasr_set_host_share.argtypes = [i32]
    L.aasr_host_usable_cores.argtypes = []
    L.aasr_host_usable_cores.restype = i32
    L.aasr_recipe_last_timing.argtypes = [vp, C.POINTER(RecipeTiming)]
    L.aasr_run_utterance.argtypes = [vp, vp, vp, i64, i32, i32, C.c_int, C.c_int,
                                     C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(i64), C.POINTER(i64)]
    L.aasr_lna_read_file.argtypes = [cp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(C.POINTER(C.c_float))]
    L.aasr_audio_decode.argtypes = [vp, vp, i64, C.POINTER(C.POINTER(C.c_int16)), C.POINTER(i64), C.POINTER(i32)]
    L.aasr_gmm_score_f64.argtypes = [vp, vp, i64, vp]
    L.aasr_gmm_get_precision.argtypes = [vp]
    L.aasr_gmm_effective_precision.argtypes = [vp]
    L.aasr_gmm_precision_states.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.aasr_free.argtypes = [vp]
    L.aasr_free.restype = None
    L.aasr_feat_get_parameters.argtypes = [vp, cp, C.POINTER(C.c_void_p), C.POINTER(i64)]
    L.aasr_feat_num_modules.argtypes = [vp]
    L.aasr_feat_module_name.argtypes = [vp, C.c_int]
    L.aasr_feat_module_name.restype = cp
    L.aasr_feat_module_type.argtypes = [vp, C.c_int]
    L.aasr_feat_module_type.restype = cp
    L.aasr_gmm_score_pitch_ok.argtypes = [vp]
    L.aasr_gmm_score_dev_pitched.argtypes = [vp, vp, i64, vp, i64, vp]
    L.aasr_lna_encode_dev_pitched.argtypes = [vp, i64, i64, i32, C.c_int, C.c_int, vp, vp, vp]
    L.aasr_lna_encode_dev_grid.argtypes = [vp, i64, i64, i32, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp]
    L.aasr_gmm_score_lna_pitched_dev.argtypes = [vp, vp, i64, vp, i64, C.c_int, C.c_int, vp, i64, vp]
    L.aasr_gmm_score_lna_overlap_active.argtypes = [vp, i64, i64, i64]
    L.aasr_gmm_score_lna_overlap_active.restype = C.c_int
    L.aasr_feat_write_config.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(i64)]
    L.aasr_recipe_read.argtypes = [cp, i32, i32, C.POINTER(C.c_void_p), C.POINTER(i64)]
    L.aasr_recipe_read_all.argtypes = [cp, i32, i32, i32, C.POINTER(C.c_void_p), C.POINTER(i64)]
    L.aasr_audio_read.argtypes = [vp, cp, C.POINTER(C.POINTER(C.c_int16)), C.POINTER(i64),
                                  C.POINTER(i32)]
    # FST decoder
    L.aasr_fstnet_create_from_file.argtypes = [cp, pvp]
    L.aasr_fstnet_destroy.argtypes = [vp]
    L.aasr_fstnet_destroy.restype = None
    for name in ("num_nodes", "num_arcs", "num_symbols", "initial", "max_pdf"):
        getattr(L, "aasr_fstnet_" + name).argtypes = [vp]
    L.aasr_fstnet_symbol.argtypes = [vp, i32]
    L.aasr_fstnet_symbol.restype = cp
    L.aasr_fstnet_arrays.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.aasr_fst_default_options.argtypes = [vp]
    L.aasr_fst_default_options.restype = None
    L.aasr_fst_durations_read.argtypes = [cp, pvp]
    L.aasr_fst_durations_destroy.argtypes = [vp]
    L.aasr_fst_durations_destroy.restype = None
    L.aasr_fst_durations_num_states.argtypes = [vp]
    L.aasr_fst_durations_logprob.argtypes = [vp, i32, i32, i32]
    L.aasr_fst_durations_logprob.restype = f
    L.aasr_fst_batch_create.argtypes = [vp, vp, vp, i32, vp, pvp]
    L.aasr_fst_batch_destroy.argtypes = [vp]
    L.aasr_fst_batch_destroy.restype = None
    L.aasr_fst_batch_device_bytes.argtypes = [vp]
    L.aasr_fst_batch_device_bytes.restype = i64
    L.aasr_fst_batch_options.argtypes = [vp, vp]
    L.aasr_fst_batch_options.restype = None
    L.aasr_fst_batch_dev.argtypes = [vp, vp, i32, i32, i64, vp, vp]
    L.aasr_fst_batch_sync.argtypes = [vp, vp, C.POINTER(i32)]
    L.aasr_fst_batch_result.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(f), C.POINTER(f), C.POINTER(f), C.POINTER(i32),
                                        vp, i32, C.POINTER(i32)]
    L.aasr_fst_batch_tokens.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp]
    L.aasr_fst_stream_create.argtypes = [vp, vp, vp, i32, i32, pvp]
    L.aasr_fst_stream_destroy.argtypes = [vp]
    L.aasr_fst_stream_destroy.restype = None
    L.aasr_fst_stream_device_bytes.argtypes = [vp]
    L.aasr_fst_stream_device_bytes.restype = i64
    L.aasr_fst_stream_options.argtypes = [vp, vp]
    L.aasr_fst_stream_options.restype = None
    L.aasr_fst_stream_reset.argtypes = [vp, i32]
    L.aasr_fst_stream_feed_dev.argtypes = [vp, vp, i32, i32, i64, vp, vp, vp]
    L.aasr_fst_stream_sync.argtypes = [vp, vp]
    L.aasr_fst_stream_result.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(f), C.POINTER(f), C.POINTER(f),
                                         C.POINTER(i32), vp, i32, C.POINTER(i32), vp, i32, C.POINTER(i32)]
    L.aasr_fst_stream_tokens.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp]
    L.aasr_fst_live_default_options.argtypes = [vp]
    L.aasr_fst_live_default_options.restype = None
    L.aasr_run_fst_live.argtypes = [vp, vp, vp, vp, vp, vp]
    L.aasr_fst_decode_default_options.argtypes = [vp]
    L.aasr_fst_decode_default_options.restype = None
    L.aasr_run_fst_decode_recipe.argtypes = [vp, vp, vp, vp, cp, vp, vp]
    L.aasr_fst_conf_default_options.argtypes = [vp]
    L.aasr_fst_conf_default_options.restype = None
    L.aasr_fst_conf_batch_create.argtypes = [vp, vp, vp, vp, i32, vp, pvp]
    L.aasr_fst_conf_batch_destroy.argtypes = [vp]
    L.aasr_fst_conf_batch_destroy.restype = None
    L.aasr_fst_conf_batch_options.argtypes = [vp, vp]
    L.aasr_fst_conf_batch_options.restype = None
    L.aasr_fst_conf_batch_dev.argtypes = [vp, vp, i32, i32, i64, vp, vp]
    L.aasr_fst_conf_batch_frame_best_dev.argtypes = [vp, vp, i32, i32, i64, vp, vp]
    L.aasr_fst_conf_batch_sync.argtypes = [vp, vp, C.POINTER(i32)]
    L.aasr_fst_conf_batch_result.argtypes = [vp, i32, vp]
    L.aasr_fst_conf_batch_grammar.argtypes = [vp]
    L.aasr_fst_conf_batch_grammar.restype = vp
    L.aasr_fst_conf_batch_phone.argtypes = [vp]
    L.aasr_fst_conf_batch_phone.restype = vp
    L.aasr_fst_conf_batch_record.argtypes = [vp, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(f), C.POINTER(f)]
    L.aasr_fst_conf_batch_frame_best.argtypes = [vp, i32, vp, vp, i32, C.POINTER(f)]
    L.aasr_fst_conf_remove_junk.argtypes = [cp, i32, cp, i32]
    L.aasr_fst_conf_remove_junk.restype = i32
    L.aasr_fst_conf_edit_distance.argtypes = [cp, i32, cp, i32]
    L.aasr_fst_conf_edit_distance.restype = i32
    L.aasr_fst_conf_formulas.argtypes = [vp, i32, cp, i32, cp, i32]
    L.aasr_fst_conf_formulas.restype = None
    L.aasr_fst_conf_stream_create.argtypes = [vp, vp, vp, vp, i32, i32, pvp]
    L.aasr_fst_conf_stream_destroy.argtypes = [vp]
    L.aasr_fst_conf_stream_destroy.restype = None
    L.aasr_fst_conf_stream_device_bytes.argtypes = [vp]
    L.aasr_fst_conf_stream_device_bytes.restype = i64
    L.aasr_fst_conf_stream_options.argtypes = [vp, vp]
    L.aasr_fst_conf_stream_options.restype = None
    L.aasr_fst_conf_stream_reset.argtypes = [vp, i32]
    L.aasr_fst_conf_stream_feed_dev.argtypes = [vp, vp, i32, i32, i64, vp, vp, vp]
    L.aasr_fst_conf_stream_sync.argtypes = [vp, vp]
    L.aasr_fst_conf_stream_result.argtypes = [vp, i32, vp]
    L.aasr_fst_conf_stream_search_result.argtypes = [vp, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(f), C.POINTER(f), C.POINTER(f),
                                                     C.POINTER(i32), vp, i32, C.POINTER(i32), vp, i32, C.POINTER(i32)]
    L.aasr_fst_conf_stream_tokens.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, i32, vp]
    L.aasr_fst_conf_stream_record.argtypes = [vp, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(f), C.POINTER(f)]
    L.aasr_fst_conf_stream_best_acu.argtypes = [vp, i32, C.POINTER(f), C.POINTER(i32)]
    L.aasr_fst_live_confidence_default_options.argtypes = [vp]
    L.aasr_fst_live_confidence_default_options.restype = None
    L.aasr_run_fst_live_confidence.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.aasr_fst_confidence_default_options.argtypes = [vp]
    L.aasr_fst_confidence_default_options.restype = None
    L.aasr_run_fst_confidence_recipe.argtypes = [vp, vp, vp, vp, vp, cp, vp, vp]


def check(status: int) -> None:
    if status != AASR_OK:
        raise AasrError(status, lib().aasr_last_error().decode("utf-8", "replace"))


def _ptr(a) -> int:
    """Address of a numpy array or torch tensor (host or device)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()


def _stream_handle(stream) -> Optional[int]:
    if stream is None:
        try:
            import torch
            if torch.cuda.is_available():
                return torch.cuda.current_stream().cuda_stream
        except Exception:
            pass
        return None
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


class Gmm:
    """Owner of an aasr_gmm handle (HmmSet scoring surface)."""

    def __init__(self, handle: int):
        self._h = handle

    @classmethod
    def from_arrays(cls, mean, var, mix_off, mix_idx, mix_w) -> "Gmm":
        mean = np.ascontiguousarray(mean, np.float64)
        var = np.ascontiguousarray(var, np.float64)
        mix_off = np.ascontiguousarray(mix_off, np.int32)
        mix_idx = np.ascontiguousarray(mix_idx, np.int32)
        mix_w = np.ascontiguousarray(mix_w, np.float64)
        h = C.c_void_p()
        check(lib().aasr_gmm_create_diag(mean.shape[1], mean.shape[0], _ptr(mean), _ptr(var),
                                         len(mix_off) - 1, _ptr(mix_off), _ptr(mix_idx),
                                         _ptr(mix_w), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_full(cls, mean, cov, mix_off, mix_idx, mix_w) -> "Gmm":
        """Full-covariance pool: cov [G, D, D]."""
        mean = np.ascontiguousarray(mean, np.float64)
        cov = np.ascontiguousarray(cov, np.float64)
        mix_off = np.ascontiguousarray(mix_off, np.int32)
        mix_idx = np.ascontiguousarray(mix_idx, np.int32)
        mix_w = np.ascontiguousarray(mix_w, np.float64)
        h = C.c_void_p()
        check(lib().aasr_gmm_create_full(mean.shape[1], mean.shape[0], _ptr(mean), _ptr(cov),
                                         len(mix_off) - 1, _ptr(mix_off), _ptr(mix_idx),
                                         _ptr(mix_w), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_files(cls, gk: str, mc: str, ph: Optional[str] = None) -> "Gmm":
        h = C.c_void_p()
        check(lib().aasr_gmm_create_from_files(gk.encode(), mc.encode(),
                                               ph.encode() if ph else None, C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_cache(cls, path: str) -> "Gmm":
        h = C.c_void_p()
        check(lib().aasr_gmm_create_from_cache(path.encode(), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_cache_checked(cls, path: str, gk: str, mc: str, ph: Optional[str] = None) -> "Gmm":
        """The cache, if it was written from exactly these text files (else AasrError 'stale')."""
        h = C.c_void_p()
        check(lib().aasr_gmm_create_from_cache_checked(path.encode(), gk.encode(), mc.encode(),
                                                       ph.encode() if ph else None, C.byref(h)))
        return cls(h.value)

    def write_cache(self, path: str) -> None:
        check(lib().aasr_gmm_write_cache(self._h, path.encode()))

    def close(self) -> None:
        if self._h:
            lib().aasr_gmm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def dim(self) -> int:
        return lib().aasr_gmm_dim(self._h)

    @property
    def num_states(self) -> int:
        return lib().aasr_gmm_num_states(self._h)

    @property
    def num_gaussians(self) -> int:
        return lib().aasr_gmm_num_gaussians(self._h)

    @property
    def expanded_rows(self) -> int:
        return lib().aasr_gmm_expanded_rows(self._h)

    def set_cmllr(self, gauss_to_transform=None, W=None) -> None:
        """W [n, D, D+1] with column 0 = bias; gauss_to_transform [G] (-1 = none).
        Call without arguments to remove the adaptation."""
        if W is None:
            check(lib().aasr_gmm_set_cmllr(self._h, 0, None, None))
            return
        W = np.ascontiguousarray(W, np.float64)
        g2t = np.ascontiguousarray(gauss_to_transform, np.int32)
        check(lib().aasr_gmm_set_cmllr(self._h, W.shape[0], _ptr(g2t), _ptr(W)))

    def score_f64(self, frames: np.ndarray) -> np.ndarray:
        """AASR_PREC_F64: double frames [F x D] -> double log state likelihoods [F x S]."""
        frames = np.ascontiguousarray(frames, np.float64)
        self._check_frames(frames)
        out = np.empty((frames.shape[0], self.num_states), np.float64)
        check(lib().aasr_gmm_score_f64(self._h, _ptr(frames), frames.shape[0], _ptr(out)))
        return out

    def read_clustering(self, path: str) -> None:
        """HmmSet::read_clustering (.gcl file)."""
        check(lib().aasr_gmm_read_clustering(self._h, path.encode()))

    def set_clustering(self, n_clusters: int, pairs=()) -> None:
        """In-memory clustering: pairs = [(gauss_index, cluster_index), ...] taken
        literally; n_clusters = 0 removes it."""
        gi = np.ascontiguousarray([p[0] for p in pairs], np.int32)
        ci = np.ascontiguousarray([p[1] for p in pairs], np.int32)
        check(lib().aasr_gmm_set_clustering(self._h, n_clusters, len(gi), _ptr(gi), _ptr(ci)))

    def cluster(self, n_clusters: int, info: int = 0) -> int:
        """gcluster on the model's own Gaussians (means and covariance diagonals), installed as read_clustering would
        install the file the tool writes; -> the number of clusters (those that kept members)."""
        check(lib().aasr_gmm_cluster(self._h, n_clusters, info))
        return self.num_clusters

    def set_clustering_min_evals(self, min_clusters: float = 1.0, min_gaussians: float = 1.0) -> None:
        """HmmSet::set_clustering_min_evals: ratios of clusters / pool Gaussians."""
        check(lib().aasr_gmm_set_clustering_min_evals(self._h, min_clusters, min_gaussians))

    @property
    def num_clusters(self) -> int:
        return lib().aasr_gmm_num_clusters(self._h)

    def cluster_exact_counts(self, n: int) -> np.ndarray:
        """Diagnostic: clusters evaluated exactly for the first n frames of the last
        clustered scoring pass."""
        L = lib()
        L.aasr_debug_cluster_exact_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        out = np.zeros(n, np.int32)
        if L.aasr_debug_cluster_exact_counts(self._h, _ptr(out), n) != 0:
            raise RuntimeError("no clustered scoring pass to report")
        return out

    def cluster_tie_frames(self) -> int:
        """Diagnostic: frames of the last clustered sub-pass settled by the priority-queue replay."""
        L = lib()
        L.aasr_debug_cluster_tie_frames.argtypes = [C.c_void_p]
        return L.aasr_debug_cluster_tie_frames(self._h)

    def set_precision(self, prec: int) -> None:
        """0 = f32, 1 = f64, 2 = f32 centred form, 3 = bf16x3 split, 4 = f16x2 split where the model is
        eligible, else bf16x3 (default)."""
        check(lib().aasr_gmm_set_precision(self._h, prec))

    def get_precision(self) -> int:
        return int(lib().aasr_gmm_get_precision(self._h))

    def effective_precision(self) -> int:
        """The arithmetic the diagonal scoring path actually runs under the current setting."""
        return int(lib().aasr_gmm_effective_precision(self._h))

    def frame_operand_ms(self, d_frames, reps: int = 10, stream=None) -> float:
        """Diagnostic: ms of one k_frame_operand launch for these frames under the current setting (< 0: not applicable)."""
        L = lib()
        L.aasr_debug_frame_operand_ms.restype = C.c_double
        L.aasr_debug_frame_operand_ms.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        return float(L.aasr_debug_frame_operand_ms(self._h, C.c_void_p(d_frames.data_ptr()), d_frames.shape[0], reps,
                                                   C.c_void_p(stream.cuda_stream if stream is not None else 0)))

    def engine_parts(self):
        """The model's engine parts (multi-pivot internal models, aasr_debug_engine_parts): a dict with `cols` (columns of
        an engine score row) and `parts`, a list of {arith (2: two fp16 terms, 3: three bf16 terms, 0: ordinary model),
        states, pivot_groups, rows}; None when the model is scored by its own layouts."""
        L = lib()
        L.aasr_debug_engine_parts.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int]
        out = (C.c_int64 * 14)()
        n = L.aasr_debug_engine_parts(self._h, out, 14)
        if n <= 0:
            return None
        return {"cols": int(out[1]),
                "parts": [{"arith": int(out[2 + 4 * i]), "states": int(out[3 + 4 * i]), "pivot_groups": int(out[4 + 4 * i]),
                           "rows": int(out[5 + 4 * i])} for i in range(n)]}

    def engine_layout(self, part: int = 0):
        """(colmap [S], col0, begin [P], real_end [P], pivots [P, dim]) of engine part `part` (aasr_debug_engine_layout);
        None when there is no such part."""
        L = lib()
        L.aasr_debug_engine_layout.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        colmap = np.zeros(self.num_states, np.int32)
        begin = np.zeros(64, np.int32)
        real_end = np.zeros(64, np.int32)
        piv = np.zeros((64, self.dim), np.float32)
        col0 = C.c_int64(0)
        n = L.aasr_debug_engine_layout(self._h, part, _ptr(colmap), _ptr(begin), _ptr(real_end), _ptr(piv), C.byref(col0))
        if n < 0:
            return None
        return colmap, int(col0.value), begin[:n].copy(), real_end[:n].copy(), piv[:n].copy()

    def engine_plan_note(self) -> str:
        L = lib()
        L.aasr_debug_engine_plan_note.argtypes = [C.c_void_p]
        L.aasr_debug_engine_plan_note.restype = C.c_char_p
        return L.aasr_debug_engine_plan_note(self._h).decode("utf-8", "replace")

    def precision_states(self):
        """(states the two-term fp16 rows cover under the current setting, states the load-time probe took out of
        that form): per-state precision routing, aasr_gmm_precision_states."""
        a, b = C.c_int64(0), C.c_int64(0)
        check(lib().aasr_gmm_precision_states(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def set_layouts(self, mask: int) -> None:
        """Diagnostic: restrict the scoring kernels the launcher may pick (bit 0
        grouped tracks, bit 1 independent tracks, 0 = general LDS-staged)."""
        L = lib()
        L.aasr_debug_set_layouts.argtypes = [C.c_void_p, C.c_int]
        L.aasr_debug_set_layouts.restype = None
        L.aasr_debug_set_layouts(self._h, mask)

    def own_layout(self) -> dict:
        """Diagnostic: the model's own one-pivot layout -- whether its two-term rows are packed, outlier routing
        (on, outlier components, states that hold them), the centred form for the whole model, states the probe moved."""
        L = lib()
        L.aasr_debug_own_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.aasr_debug_own_layout.restype = None
        out = (C.c_int64 * 6)()
        L.aasr_debug_own_layout(self._h, out)
        return {"two_term_rows": bool(out[0]), "routing": bool(out[1]), "outlier_comps": int(out[2]),
                "outlier_states": int(out[3]), "all_centred": bool(out[4]), "probe_moved": int(out[5])}

    def outlier_path(self):
        """Diagnostic: (launches of the scoring kernel that merged the outlier components itself, runs of the merge
        pass) over the scoring calls on this handle so far."""
        L = lib()
        L.aasr_debug_outlier_path.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.aasr_debug_outlier_path.restype = None
        out = (C.c_int64 * 2)()
        L.aasr_debug_outlier_path(self._h, out)
        return int(out[0]), int(out[1])

    def set_outlier_fuse(self, on: bool) -> None:
        """Diagnostic: False leaves the outlier components of every call to the merge pass."""
        L = lib()
        L.aasr_debug_set_outlier_fuse.argtypes = [C.c_void_p, C.c_int]
        L.aasr_debug_set_outlier_fuse.restype = None
        L.aasr_debug_set_outlier_fuse(self._h, 1 if on else 0)

    def active_layout(self) -> int:
        L = lib()
        L.aasr_debug_active_layout.argtypes = [C.c_void_p]
        return L.aasr_debug_active_layout(self._h)

    def _check_frames(self, frames) -> None:
        # the C ABI takes a pointer and a frame count: the row width is the caller's promise
        if frames.ndim != 2 or frames.shape[1] != self.dim:
            raise ValueError("frames must be [F x %d], got %s" % (self.dim, tuple(frames.shape)))

    def score(self, frames: np.ndarray) -> np.ndarray:
        frames = np.ascontiguousarray(frames, np.float32)
        self._check_frames(frames)
        out = np.empty((frames.shape[0], self.num_states), np.float32)
        check(lib().aasr_gmm_score(self._h, _ptr(frames), frames.shape[0], _ptr(out)))
        return out

    def score_dev(self, d_frames, d_out, stream=None) -> None:
        check(lib().aasr_gmm_score_dev(self._h, _ptr(d_frames), d_frames.shape[0], _ptr(d_out),
                                       _stream_handle(stream)))

    def score_scratch_floats(self, F: int) -> int:
        return lib().aasr_gmm_score_scratch_floats(self._h, F)

    def score_lna_dev(self, d_frames, d_scratch, d_bytes, normalize: bool = True, lnabytes: int = 2, stream=None) -> None:
        """Frames (device) -> packed LNA rows (device) through the engine's own intermediate layout."""
        check(lib().aasr_gmm_score_lna_dev(self._h, d_frames.data_ptr(), d_frames.shape[0], int(normalize), lnabytes,
                                           d_scratch.data_ptr(), d_bytes.data_ptr(), _stream_handle(stream)))

    def score_pitch_ok(self) -> bool:
        """Whether score_dev_pitched accepts a row pitch other than the state count."""
        return bool(lib().aasr_gmm_score_pitch_ok(self._h))

    def score_dev_pitched(self, d_frames, d_out, pitch: int, stream=None) -> None:
        """d_out: device buffer of frames x pitch floats (pitch >= states)."""
        check(lib().aasr_gmm_score_dev_pitched(self._h, _ptr(d_frames), d_frames.shape[0], _ptr(d_out),
                                               pitch, _stream_handle(stream)))

    def score_lna_dev_pitched(self, d_frames, d_scores, pitch: int, d_bytes, normalize: bool = True, lnabytes: int = 2,
                              chunk_frames: int = 0, stream=None) -> None:
        """score_dev_pitched + lna_encode_dev in one call: the LNA pass of a frame chunk runs beside the scoring of the
        next chunk where the model allows it (score_lna_overlap_active), the plain sequence otherwise; same results."""
        check(lib().aasr_gmm_score_lna_pitched_dev(self._h, _ptr(d_frames), d_frames.shape[0], _ptr(d_scores), pitch,
                                                   int(normalize), lnabytes, _ptr(d_bytes), chunk_frames,
                                                   _stream_handle(stream)))

    def score_lna_overlap_active(self, n_frames: int, pitch: int, chunk_frames: int = 0) -> bool:
        return bool(lib().aasr_gmm_score_lna_overlap_active(self._h, n_frames, pitch, chunk_frames))

    def gauss_loglik(self, frames: np.ndarray) -> np.ndarray:
        frames = np.ascontiguousarray(frames, np.float32)
        self._check_frames(frames)
        out = np.empty((frames.shape[0], self.num_gaussians), np.float32)
        check(lib().aasr_gmm_gauss_loglik(self._h, _ptr(frames), frames.shape[0], _ptr(out)))
        return out


def lna_encode(state_loglik: np.ndarray, normalize: bool = True, lnabytes: int = 2):
    x = np.ascontiguousarray(state_loglik, np.float32)
    F, S = x.shape
    lp = np.empty((F, S), np.float32)
    by = np.empty((F, S * lnabytes), np.uint8)
    check(lib().aasr_lna_encode(_ptr(x), F, S, int(normalize), lnabytes, _ptr(lp), _ptr(by)))
    return lp, by


def lna_encode_dev(d_loglik, normalize: bool, lnabytes: int, d_lp=None, d_bytes=None, stream=None,
                   num_states: Optional[int] = None, colmap=None, wgs_per_cu: Optional[int] = None):
    """d_loglik: [F x S], or [F x pitch] with num_states = S < pitch (padded rows).
    colmap (device int32 [S]: state i sits in column colmap[i]) and wgs_per_cu (the grid of the register-resident
    kernels, the library's 32 when only the map is given) go through aasr_lna_encode_dev_grid."""
    F, P = d_loglik.shape
    if colmap is not None or wgs_per_cu is not None:
        check(lib().aasr_lna_encode_dev_grid(_ptr(d_loglik), P, F, P if num_states is None else num_states,
                                             int(normalize), lnabytes, _ptr(colmap),
                                             32 if wgs_per_cu is None else wgs_per_cu, _ptr(d_lp), _ptr(d_bytes),
                                             _stream_handle(stream)))
    elif num_states is None or num_states == P:
        check(lib().aasr_lna_encode_dev(_ptr(d_loglik), F, P, int(normalize), lnabytes, _ptr(d_lp),
                                        _ptr(d_bytes), _stream_handle(stream)))
    else:
        check(lib().aasr_lna_encode_dev_pitched(_ptr(d_loglik), P, F, num_states, int(normalize), lnabytes,
                                                _ptr(d_lp), _ptr(d_bytes), _stream_handle(stream)))


def lna_header(num_states: int, lnabytes: int) -> bytes:
    buf = (C.c_uint8 * 5)()
    lib().aasr_lna_header(num_states, lnabytes, buf)
    return bytes(buf)


class Feat:
    """Owner of an aasr_feat handle (FeatureGenerator surface)."""

    def __init__(self, cfg_text: str):
        h = C.c_void_p()
        check(lib().aasr_feat_create(cfg_text.encode(), C.byref(h)))
        self._h = h.value

    @classmethod
    def from_file(cls, path: str) -> "Feat":
        return cls(open(path).read())

    def write_config(self) -> str:
        """FeatureGenerator::write_configuration: the graph as .cfg text."""
        out = C.c_void_p()
        n = C.c_int64()
        check(lib().aasr_feat_write_config(self._h, C.byref(out), C.byref(n)))
        try:
            return C.string_at(out, n.value).decode()
        finally:
            lib().aasr_free(out)

    def close(self) -> None:
        if self._h:
            lib().aasr_feat_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def dim(self) -> int:
        return lib().aasr_feat_dim(self._h)

    @property
    def frame_rate(self) -> float:
        return lib().aasr_feat_frame_rate(self._h)

    @property
    def sample_rate(self) -> int:
        return lib().aasr_feat_sample_rate(self._h)

    def module_dim(self, name: str) -> int:
        return lib().aasr_feat_module_dim(self._h, name.encode())

    def halo(self):
        l, r = C.c_int(), C.c_int()
        lib().aasr_feat_halo(self._h, C.byref(l), C.byref(r))
        return l.value, r.value

    def last_frame(self, n_samples: int) -> int:
        return lib().aasr_feat_last_frame(self._h, n_samples)

    def eof_frame(self, n_samples: int) -> int:
        """first frame whose window crosses the end of the input = frames a whole-file run emits"""
        return lib().aasr_feat_eof_frame(self._h, n_samples)

    def run(self, pcm: np.ndarray, first_frame: int, n_frames: int, module: Optional[str] = None,
            dtype=np.float32) -> np.ndarray:
        pcm = np.ascontiguousarray(pcm, np.int16)
        dim = self.module_dim(module) if module else self.dim
        if dim < 0:
            raise AasrError(AASR_ERR_INVALID, "unknown module requested: %s" % module)
        out = np.empty((n_frames, dim), dtype)
        fn = lib().aasr_feat_run if dtype == np.float32 else lib().aasr_feat_run_f64
        check(fn(self._h, _ptr(pcm), len(pcm), first_frame, n_frames,
                 module.encode() if module else None, _ptr(out)))
        return out

    def run_features(self, frames: np.ndarray, first_frame: int, n_frames: int,
                     module: Optional[str] = None, dtype=np.float32) -> np.ndarray:
        """Graphs with a `pre` base module: float feature frames [N x dim] in."""
        frames = np.ascontiguousarray(frames, np.float32)
        dim = self.module_dim(module) if module else self.dim
        out = np.empty((n_frames, dim), dtype)
        fn = lib().aasr_feat_run_features if dtype == np.float32 else lib().aasr_feat_run_features_f64
        check(fn(self._h, _ptr(frames), frames.size, first_frame, n_frames,
                 module.encode() if module else None, _ptr(out)))
        return out

    def run_batch_dev(self, d_pcm, pcm_off: np.ndarray, frame_off: np.ndarray, d_out, stream=None):
        pcm_off = np.ascontiguousarray(pcm_off, np.int64)
        frame_off = np.ascontiguousarray(frame_off, np.int64)
        check(lib().aasr_feat_run_batch_dev(self._h, _ptr(d_pcm), _ptr(pcm_off), _ptr(frame_off),
                                            len(pcm_off) - 1, _ptr(d_out), _stream_handle(stream)))

    def set_parameters(self, module: str, block_text: str) -> None:
        check(lib().aasr_feat_set_parameters(self._h, module.encode(), block_text.encode()))

    def get_parameters(self, module: str) -> str:
        """FeatureModule::get_parameters as a "{ name value ... }" block."""
        out = C.c_void_p()
        n = C.c_int64()
        check(lib().aasr_feat_get_parameters(self._h, module.encode(), C.byref(out), C.byref(n)))
        try:
            return C.string_at(out, n.value).decode()
        finally:
            lib().aasr_free(out)

    def modules(self):
        """[(name, type)] in configuration order."""
        L = lib()
        return [(L.aasr_feat_module_name(self._h, i).decode(), L.aasr_feat_module_type(self._h, i).decode())
                for i in range(L.aasr_feat_num_modules(self._h))]


def recipe_batch_range(total: int, num_batches: int, batch_index: int):
    f, n = C.c_int32(), C.c_int32()
    check(lib().aasr_recipe_batch_range(total, num_batches, batch_index, C.byref(f), C.byref(n)))
    return f.value, n.value


def debug_feat_fusion(on: bool) -> None:
    """Diagnostic: False = every feature module runs its own kernel (the fused kernels must match it
    bit for bit)."""
    L = lib()
    L.aasr_debug_feat_fusion.argtypes = [C.c_int]
    L.aasr_debug_feat_fusion.restype = None
    L.aasr_debug_feat_fusion(int(on))


def debug_cluster_heap(on: bool) -> None:
    """Diagnostic: send every frame's cluster selection through the priority-queue replay."""
    L = lib()
    L.aasr_debug_cluster_heap.argtypes = [C.c_int]
    L.aasr_debug_cluster_heap.restype = None
    L.aasr_debug_cluster_heap(int(on))


def debug_lna_frames_per_pass(q: int) -> None:
    """Diagnostic: frame rows per workgroup pass of later LNA launches of this process -- 1: the one-frame kernel, 2 or 4:
    the multi-frame kernel where a call qualifies (2-byte codes, no float output, no column map, S in the <13> range);
    negative: the compiled-in value.  The bytes do not depend on it."""
    if q >= 0 and q not in (1, 2, 4):
        raise ValueError("frames per pass: 1, 2, 4 or a negative value, got %r" % (q,))
    L = lib()
    L.aasr_debug_lna_frames_per_pass.argtypes = [C.c_int]
    L.aasr_debug_lna_frames_per_pass.restype = None
    L.aasr_debug_lna_frames_per_pass(int(q))


def recipe_frame_limits(start_time: float, end_time: float, frame_rate: float):
    """(start_frame, end_frame) of aku/phone_probs.cc:199-206, float arithmetic."""
    a, b = C.c_int32(), C.c_int32()
    lib().aasr_recipe_frame_limits(start_time, end_time, frame_rate, C.byref(a), C.byref(b))
    return a.value, b.value


def recipe_read(text, num_batches: int = 0, batch_index: int = 0):
    """Recipe::read on the host: list of (audio, lna, speaker, utterance, start_time, end_time)."""
    out = C.c_void_p()
    n = C.c_int64()
    raw = text if isinstance(text, bytes) else text.encode()
    check(lib().aasr_recipe_read(raw, num_batches, batch_index, C.byref(out), C.byref(n)))
    try:
        table = C.string_at(out, n.value)
    finally:
        lib().aasr_free(out)
    rows = []
    for line in table.split(b"\n")[:-1]:
        f = line.split(b"\x1f")
        # the times are float fields printed with 9 significant digits: exact through float32
        rows.append(tuple(x.decode("latin-1") for x in f[:4]) +
                    (float(np.float32(float(f[4]))), float(np.float32(float(f[5])))))
    return rows


def recipe_read_all(text, num_batches: int = 0, batch_index: int = 0, cluster_speakers: bool = False):
    """Recipe::read with every Info field: list of 13-tuples (audio, alt-audio, transcript,
    alignment, hmmnet, den-hmmnet, lna, start_time, end_time, start_line, end_line, speaker,
    utterance)."""
    out = C.c_void_p()
    n = C.c_int64()
    raw = text if isinstance(text, bytes) else text.encode()
    check(lib().aasr_recipe_read_all(raw, num_batches, batch_index, int(cluster_speakers), C.byref(out), C.byref(n)))
    try:
        table = C.string_at(out, n.value)
    finally:
        lib().aasr_free(out)
    rows = []
    for line in table.split(b"\n")[:-1]:
        f = [x.decode("latin-1") for x in line.split(b"\x1f")]
        rows.append(tuple(f[:7]) + (float(np.float32(float(f[7]))), float(np.float32(float(f[8]))),
                                    int(f[9]), int(f[10]), f[11], f[12]))
    return rows


def lna_read_file(path: str):
    """LnaReaderCircular's view of an LNA file (1-, 2- or 4-byte): (float32 [frames x states], lnabytes)."""
    out = C.POINTER(C.c_float)()
    S = C.c_int32()
    nb = C.c_int32()
    F = C.c_int64()
    check(lib().aasr_lna_read_file(path.encode(), C.byref(S), C.byref(nb), C.byref(F), C.byref(out)))
    try:
        n = F.value * S.value
        lp = np.ctypeslib.as_array(out, shape=(max(n, 1),))[:n].copy().reshape(F.value, S.value)
    finally:
        lib().aasr_free(out)
    return lp, nb.value


def audio_read(path: str, feat: Optional["Feat"] = None):
    """AudioReader::open + read (host only).  Returns (int16 samples, sample rate)."""
    out = C.POINTER(C.c_int16)()
    n = C.c_int64()
    rate = C.c_int32()
    check(lib().aasr_audio_read(feat._h if feat is not None else None, path.encode(), C.byref(out),
                                C.byref(n), C.byref(rate)))
    try:
        pcm = np.ctypeslib.as_array(out, shape=(max(n.value, 1),))[:n.value].copy()
    finally:
        lib().aasr_free(out)
    return pcm, rate.value


def audio_decode(data: bytes, feat: Optional["Feat"] = None):
    """aasr_audio_decode: the file decoding of audio_read for bytes already in memory."""
    out = C.POINTER(C.c_int16)()
    n = C.c_int64()
    rate = C.c_int32()
    buf = C.create_string_buffer(data, len(data))
    check(lib().aasr_audio_decode(feat._h if feat is not None else None, C.cast(buf, C.c_void_p), len(data),
                                  C.byref(out), C.byref(n), C.byref(rate)))
    try:
        pcm = np.ctypeslib.as_array(out, shape=(max(n.value, 1),))[:n.value].copy()
    finally:
        lib().aasr_free(out)
    return pcm, rate.value


def run_utterance(feat: Feat, gmm: Gmm, pcm: np.ndarray, start_frame: int = 0, end_frame: int = 0,
                  normalize: bool = True, lnabytes: int = 2):
    """Returns (lna file image as bytes, number of frames)."""
    pcm = np.ascontiguousarray(pcm, np.int16)
    out = C.POINTER(C.c_uint8)()
    n = C.c_int64()
    frames = C.c_int64()
    check(lib().aasr_run_utterance(feat._h, gmm._h, _ptr(pcm), len(pcm), start_frame, end_frame,
                                   int(normalize), lnabytes, C.byref(out), C.byref(n), C.byref(frames)))
    try:
        data = C.string_at(out, n.value)
    finally:
        lib().aasr_free(out)
    return data, frames.value


class SpeakerConfig:
    """aku::SpeakerConfig on the engine's handles (aasr_spkc_*)."""

    def __init__(self, feat: "Feat", gmm: Optional["Gmm"] = None):
        self._h = C.c_void_p()
        self._keep = (feat, gmm)
        check(lib().aasr_spkc_create(feat._h, gmm._h if gmm is not None else None, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.aasr_spkc_destroy(self._h)
            self._h = None

    def set_model(self, gmm: "Gmm") -> None:
        self._keep = (self._keep[0], gmm)
        check(lib().aasr_spkc_set_model(self._h, gmm._h))

    def read_file(self, path: str) -> None:
        check(lib().aasr_spkc_read_file(self._h, path.encode()))

    def read_text(self, text: str) -> None:
        check(lib().aasr_spkc_read_text(self._h, text.encode()))

    def set_speaker(self, speaker_id: str = "") -> None:
        check(lib().aasr_spkc_set_speaker(self._h, speaker_id.encode()))

    def set_utterance(self, utterance_id: str = "") -> None:
        check(lib().aasr_spkc_set_utterance(self._h, utterance_id.encode()))

    @property
    def num_changes(self) -> int:
        return lib().aasr_spkc_num_changes(self._h)

    def write_text(self, speakers=None, utterances=None) -> str:
        """SpeakerConfig::write_speaker_file as text; speakers / utterances: lists of ids to keep (None: all)."""
        def arr(ids):
            if ids is None:
                return None, -1
            a = (C.c_char_p * max(1, len(ids)))(*[i.encode() for i in ids])
            return a, len(ids)
        sp, n_sp = arr(speakers)
        ut, n_ut = arr(utterances)
        out, n = C.c_void_p(), C.c_int64()
        check(lib().aasr_spkc_write_text(self._h, sp, n_sp, ut, n_ut, C.byref(out), C.byref(n)))
        try:
            return C.string_at(out, n.value).decode()
        finally:
            lib().aasr_free(out)


def run_recipe(feat: Feat, gmm: Gmm, recipe_path: str, lnabytes: int = 2, normalize: bool = True,
               num_batches: int = 0, batch_index: int = 0, no_overwrite: bool = False,
               raw_audio: bool = False, info: int = 0, afname: bool = False,
               out_dir: Optional[str] = None, speakers: Optional[SpeakerConfig] = None,
               sort_recipe: bool = False) -> RunStats:
    opt = RunOptions(lnabytes, int(normalize), num_batches, batch_index, int(no_overwrite),
                     int(raw_audio), info, int(afname), out_dir.encode() if out_dir else None,
                     speakers._h if speakers is not None else None, int(sort_recipe))
    st = RunStats()
    check(lib().aasr_run_recipe(feat._h, gmm._h, recipe_path.encode(), C.byref(opt), C.byref(st)))
    return st


def recipe_last_timing(gmm: Gmm) -> dict:
    t = RecipeTiming()
    check(lib().aasr_recipe_last_timing(gmm._h, C.byref(t)))
    return t.as_dict()


def set_host_share(processes: int) -> None:
    check(lib().aasr_set_host_share(int(processes)))


# ---- forced alignment ---------------------------------------------------------------------------

class AlignOptions(C.Structure):
    """aasr_align_options: align's options (aku/align.cc:180-198) with the same defaults."""
    _fields_ = [("swins", C.c_int32), ("beam", C.c_double), ("sbeam", C.c_int32), ("maxbeam", C.c_double),
                ("overlap", C.c_float), ("no_force_end", C.c_int32), ("phoseg", C.c_int32), ("info", C.c_int32),
                ("num_batches", C.c_int32), ("batch_index", C.c_int32), ("speakers", C.c_void_p)]

    @classmethod
    def defaults(cls, **kw) -> "AlignOptions":
        o = cls()
        lib().aasr_align_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


ALIGN_ACTIVE, ALIGN_OK, ALIGN_GAVE_UP, ALIGN_ERROR = 0, 1, 2, 3


class Topology:
    """Owner of an aasr_topo handle: the HMMs of a .ph file with their transitions."""

    def __init__(self, ph_path: str):
        h = C.c_void_p()
        check(lib().aasr_topo_create_from_ph(ph_path.encode(), C.byref(h)))
        self._h = h.value

    def close(self) -> None:
        if self._h:
            lib().aasr_topo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self) -> int:
        return self._h

    def num_hmms(self) -> int:
        return lib().aasr_topo_num_hmms(self._h)

    def hmm_index(self, label: str) -> int:
        return lib().aasr_topo_hmm_index(self._h, label.encode())

    def hmm_label(self, hmm: int) -> str:
        return lib().aasr_topo_hmm_label(self._h, hmm).decode()

    def hmm_states(self, hmm: int) -> list:
        n = lib().aasr_topo_hmm_num_states(self._h, hmm)
        out = np.zeros(max(n, 1), np.int32)
        check(lib().aasr_topo_hmm_states(self._h, hmm, _ptr(out)))
        return [int(x) for x in out[:n]]

    def num_states(self) -> int:
        return lib().aasr_topo_num_states(self._h)

    def transitions(self, state: int) -> list:
        """[(target_offset, prob)] of a state, in file order."""
        n = lib().aasr_topo_state_num_transitions(self._h, state)
        off = np.zeros(max(n, 1), np.int32)
        prob = np.zeros(max(n, 1), np.float64)
        check(lib().aasr_topo_state_transitions(self._h, state, _ptr(off), _ptr(prob)))
        return [(int(off[k]), float(prob[k])) for k in range(n)]

    def max_offset(self) -> int:
        return lib().aasr_topo_max_offset(self._h)

    def validate(self, gmm: "Gmm") -> None:
        check(lib().aasr_topo_validate(self._h, gmm._h))

    def check_states(self, num_states: int) -> None:
        check(lib().aasr_topo_check_states(self._h, num_states))

    def read_transcript(self, path: str, frame_rate: float = 125.0, first_frame: int = 0, last_frame: int = 0) -> list:
        """HMM index per transcript line (-1: a line that adds none)."""
        p = C.POINTER(C.c_int32)()
        n = C.c_int32()
        check(lib().aasr_align_read_transcript(self._h, path.encode(), frame_rate, first_frame, last_frame,
                                               C.byref(p), C.byref(n)))
        try:
            return [int(p[k]) for k in range(n.value)]
        finally:
            lib().aasr_free(p)


def align_format_line(frame_rate: float, start: int, end: int, label: str, comment: str) -> str:
    buf = C.create_string_buffer(4096)
    n = lib().aasr_align_format_line(frame_rate, start, end, label.encode(), comment.encode(), buf, len(buf))
    if n < 0:
        raise AasrError(AASR_ERR_INVALID, "line too long")
    return buf.raw[:n].decode()


def align_batch(gmm: "Gmm", topo: Topology, transcripts: list, scores, row0: list, start_frames: list,
                end_frames: list, eof_frames: list, opts: Optional[AlignOptions] = None, windows: int = 1 << 20,
                stream: int = 0) -> list:
    """Batched forced alignment on the device.  transcripts[u]: HMM index per line; scores: a device
    tensor of state log-likelihood rows (float32, or float64 for AASR_PREC_F64 rows), row0[u] the row of
    utterance u's first frame.  Enqueues `windows` window steps per call until every utterance is done.
    Returns per utterance a dict: positions (committed absolute transcription position per frame),
    loglik, status, n_fail."""
    L = lib()
    opts = opts or AlignOptions.defaults()
    n = len(transcripts)
    line_off = np.zeros(n + 1, np.int32)
    for u, t in enumerate(transcripts):
        line_off[u + 1] = line_off[u] + len(t)
    lines = np.ascontiguousarray(np.concatenate([np.asarray(t, np.int32) for t in transcripts] + [np.zeros(1, np.int32)]))
    sf = np.ascontiguousarray(start_frames, np.int32)
    ef = np.ascontiguousarray(end_frames, np.int32)
    of = np.ascontiguousarray(eof_frames, np.int32)
    r0 = np.ascontiguousarray(row0, np.int64)
    b = C.c_void_p()
    check(L.aasr_align_batch_create(topo.handle, C.byref(opts), n, _ptr(line_off), _ptr(lines), _ptr(sf), _ptr(ef),
                                    _ptr(of), C.byref(b)))
    try:
        f64 = 1 if str(scores.dtype) == "torch.float64" else 0
        pitch = scores.shape[1]
        active = C.c_int32(n)
        steps = 0
        while active.value > 0:
            check(L.aasr_align_batch_dev(gmm._h, b, _ptr(scores), pitch, f64, _ptr(r0), windows, stream))
            check(L.aasr_align_batch_sync(b, stream, C.byref(active)))
            steps += 1
        out = []
        for u in range(n):
            rows = L.aasr_align_batch_rows(b, u)
            pos = np.zeros(max(rows, 1), np.int32)
            nc, st, nf = C.c_int32(), C.c_int32(), C.c_int32()
            ll = C.c_double()
            check(L.aasr_align_batch_result(b, u, _ptr(pos), C.byref(nc), C.byref(ll), C.byref(st), C.byref(nf)))
            out.append({"positions": pos[:nc.value].copy(), "loglik": ll.value, "status": st.value,
                        "n_fail": nf.value, "calls": steps})
        return out
    finally:
        L.aasr_align_batch_destroy(b)


# ---- ML statistics ------------------------------------------------------------------------------

class StatsOptions(C.Structure):
    """aasr_stats_options: stats' options (aku/stats.cc:321-356) for --ml over .phn files."""
    _fields_ = [("transitions", C.c_int32), ("ophn", C.c_int32), ("no_train", C.c_int32), ("uttadap", C.c_int32),
                ("info", C.c_int32), ("num_batches", C.c_int32), ("batch_index", C.c_int32),
                ("speakers", C.c_void_p), ("out", C.c_char_p), ("full_stats", C.c_int32)]

    @classmethod
    def defaults(cls, **kw) -> "StatsOptions":
        o = cls()
        lib().aasr_stats_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def stats_read_segmentation(topo: Topology, path: str, frame_rate: float = 125.0, first_frame: int = 0,
                            last_frame: int = 0, eof_frame: int = -1, transitions: bool = True):
    """PhnReader::next_frame as stats drives it (host only).  Returns (start_frame, pdf per frame, global
    transition index per frame or -1), or None for a file without lines."""
    L = lib()
    sf, n = C.c_int32(), C.c_int32()
    pp, tp = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
    check(L.aasr_stats_read_segmentation(topo.handle, path.encode(), frame_rate, first_frame, last_frame, eof_frame,
                                         1 if transitions else 0, C.byref(sf), C.byref(pp), C.byref(tp), C.byref(n)))
    try:
        if n.value < 0:
            return None
        pdf = np.array([pp[k] for k in range(n.value)], np.int32)
        tr = np.array([tp[k] for k in range(n.value)], np.int32)
        return sf.value, pdf, tr
    finally:
        L.aasr_free(pp)
        L.aasr_free(tp)


def stats_write_gks(path: str, feacount, gamma, aux_gamma, sum_x, sum_xx, mode: int = 1) -> None:
    fc = np.ascontiguousarray(feacount, np.int64)
    g, a = np.ascontiguousarray(gamma, np.float64), np.ascontiguousarray(aux_gamma, np.float64)
    sx, sxx = np.ascontiguousarray(sum_x, np.float64), np.ascontiguousarray(sum_xx, np.float64)
    G, D = sx.shape
    check(lib().aasr_stats_write_gks(path.encode(), G, D, mode, _ptr(fc), _ptr(g), _ptr(a), _ptr(sx), _ptr(sxx)))


def stats_write_gks_full(path: str, feacount, gamma, aux_gamma, sum_x, sum_xx_packed) -> None:
    """The mode-3 .gks: sum_xx_packed [G x D (D + 1) / 2], the lower triangles row by row (j <= i)."""
    fc = np.ascontiguousarray(feacount, np.int64)
    g, a = np.ascontiguousarray(gamma, np.float64), np.ascontiguousarray(aux_gamma, np.float64)
    sx, sxx = np.ascontiguousarray(sum_x, np.float64), np.ascontiguousarray(sum_xx_packed, np.float64)
    G, D = sx.shape
    if sxx.shape != (G, D * (D + 1) // 2):
        raise ValueError("sum_xx_packed must be [%d x %d]" % (G, D * (D + 1) // 2))
    check(lib().aasr_stats_write_gks_full(path.encode(), G, D, _ptr(fc), _ptr(g), _ptr(a), _ptr(sx), _ptr(sxx)))


def stats_write_mcs(path: str, mix_off, mix_idx, count, gamma, aux_gamma, mixture_ll, mode: int = 1) -> None:
    off, idx = np.ascontiguousarray(mix_off, np.int32), np.ascontiguousarray(mix_idx, np.int32)
    cnt, g = np.ascontiguousarray(count, np.int64), np.ascontiguousarray(gamma, np.float64)
    a, mll = np.ascontiguousarray(aux_gamma, np.float64), np.ascontiguousarray(mixture_ll, np.float64)
    check(lib().aasr_stats_write_mcs(path.encode(), len(off) - 1, mode, _ptr(off), _ptr(idx), _ptr(cnt), _ptr(g),
                                     _ptr(a), _ptr(mll)))


def stats_write_phs(path: str, source, target_offset, count) -> None:
    src, off = np.ascontiguousarray(source, np.int32), np.ascontiguousarray(target_offset, np.int32)
    cnt = np.ascontiguousarray(count, np.float64)
    check(lib().aasr_stats_write_phs(path.encode(), len(src), _ptr(src), _ptr(off), _ptr(cnt)))


def stats_write_lls(path: str, loglik: float, frames: int) -> None:
    check(lib().aasr_stats_write_lls(path.encode(), loglik, frames))


class Stats:
    """Owner of an aasr_stats handle: ML statistics of one model and topology, accumulated on the device."""

    def __init__(self, gmm: "Gmm", topo: Topology, n_components: int = 0, full: bool = False):
        """n_components: the model's mixture components in all (for the per-component gammas of fetch); full: collect
        the full second moments as well (mode-3 dumps)"""
        h = C.c_void_p()
        L = lib()
        check((L.aasr_stats_create_full if full else L.aasr_stats_create)(gmm._h, topo.handle, C.byref(h)))
        self._h = h.value
        self.full = bool(full)
        self.G, self.D, self.S, self.K = gmm.num_gaussians, gmm.dim, gmm.num_states, n_components

    def close(self) -> None:
        if self._h:
            lib().aasr_stats_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def accumulate_dev(self, d_frames, pdf, d_frame_ll=None, stream=None) -> None:
        """d_frames: a float64 device tensor [n x dim]; pdf: host int32 per frame (-1: skip)."""
        p = np.ascontiguousarray(pdf, np.int32)
        check(lib().aasr_stats_accumulate_dev(self._h, _ptr(d_frames), len(p), _ptr(p), _ptr(d_frame_ll),
                                              _stream_handle(stream)))

    def accumulate_weighted_dev(self, d_frames, cnt, d_rows, d_weights, stream=None) -> None:
        """Weighted entries: cnt (host int64, states + 1) the first entry of every pdf in d_rows (int32 device tensor)
        and d_weights (float64 device tensor); d_frames a float64 device tensor [n x dim]."""
        c = np.ascontiguousarray(cnt, np.int64)
        if len(c) != self.S + 1:
            raise ValueError("cnt must have %d entries" % (self.S + 1))
        check(lib().aasr_stats_accumulate_weighted_dev(self._h, _ptr(d_frames), int(d_frames.shape[0]), _ptr(c), _ptr(d_rows),
                                                       _ptr(d_weights), _stream_handle(stream)))

    def launch_shape(self) -> dict:
        """Diagnostic: the shape of the accumulation kernel's launch in the last accumulate_dev call that launched it
        (zeros before the first): its dimension instance, frames per sub-block, whether the mixture records were staged
        in LDS, the model's largest mixture and the work items."""
        L = lib()
        L.aasr_debug_stats_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.aasr_debug_stats_shape.restype = None
        out = (C.c_int32 * 5)()
        L.aasr_debug_stats_shape(self._h, out)
        return {"dimp": int(out[0]), "block": int(out[1]), "lds_recs": int(out[2]), "max_comps": int(out[3]),
                "items": int(out[4])}

    def mode(self) -> int:
        return int(lib().aasr_stats_mode(self._h))

    def full_launch_shape(self) -> dict:
        """Diagnostic: the full pass of the last accumulate_dev call that reached it (zeros before, and on a plain
        handle): PB, work items, launches and units (item x component)."""
        out = (C.c_int32 * 4)()
        lib().aasr_debug_stats_full_shape(self._h, out)
        return {"pb": int(out[0]), "items": int(out[1]), "launches": int(out[2]), "units": int(out[3])}

    def set_slab_bytes(self, nbytes: int) -> None:
        """Diagnostic: the bound on a launch's slab memory in the full pass (the result does not depend on it)."""
        check(lib().aasr_debug_stats_set_slab_bytes(self._h, int(nbytes)))

    def add_transitions(self, transition) -> None:
        t = np.ascontiguousarray(transition, np.int32)
        check(lib().aasr_stats_add_transitions(self._h, _ptr(t), len(t)))

    def fetch(self, stream=None) -> dict:
        """Waits for the device and returns every sum: per pool Gaussian feacount, gamma, aux_gamma,
        sum_x, sum_xx; per pdf count and mixture_ll; per mixture component (record order) mix_gamma."""
        L = lib()
        check(L.aasr_stats_fetch(self._h, _stream_handle(stream)))
        G, D, S = self.G, self.D, self.S
        fc = np.zeros(G, np.int64)
        g, a = np.zeros(G), np.zeros(G)
        sx, sxx = np.zeros((G, D)), np.zeros((G, D))
        check(L.aasr_stats_gaussians(self._h, _ptr(fc), _ptr(g), _ptr(a), _ptr(sx), _ptr(sxx)))
        cnt, mll, mg = np.zeros(S, np.int64), np.zeros(S), np.zeros(max(1, self.K))
        check(L.aasr_stats_mixtures(self._h, _ptr(cnt), _ptr(mg), _ptr(mll)))
        out = {"feacount": fc, "gamma": g, "aux_gamma": a, "sum_x": sx, "sum_xx": sxx, "count": cnt,
               "mixture_ll": mll, "mix_gamma": mg[:self.K]}
        if self.full:   # the packed lower triangles of sum gamma x x^T, row-major with j <= i
            out["sum_xx_full"] = np.zeros((G, D * (D + 1) // 2))
            check(L.aasr_stats_full_moments(self._h, _ptr(out["sum_xx_full"])))
        return out

    def transitions(self):
        n = lib().aasr_stats_num_transitions(self._h)
        src, off, cnt = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1))
        check(lib().aasr_stats_transitions(self._h, _ptr(src), _ptr(off), _ptr(cnt)))
        return src[:n], off[:n], cnt[:n]

    def write(self, base: str) -> None:
        check(lib().aasr_stats_write(self._h, base.encode()))


class StatsNetworkOptions(C.Structure):
    """aasr_stats_network_options: what stats --networks adds (-M vit, -F, -W, -A, -a)."""
    _fields_ = [("viterbi", C.c_int32), ("ac_scale_given", C.c_int32), ("fw_beam", C.c_double), ("bw_beam", C.c_double),
                ("ac_scale", C.c_double), ("alignment", C.c_int32)]

    @classmethod
    def defaults(cls, **kw) -> "StatsNetworkOptions":
        o = cls()
        lib().aasr_stats_network_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def run_stats_recipe(feat: "Feat", gmm: "Gmm", topo: Topology, recipe_path: str, out: str,
                     opts: Optional[StatsOptions] = None, networks: Optional[StatsNetworkOptions] = None) -> dict:
    """stats over a recipe; with `networks` Baum-Welch over the recipe's hmmnet= networks (stats --networks)"""
    opts = opts or StatsOptions.defaults()
    ob = out.encode()
    opts.out = ob
    st = RunStats()
    L = lib()
    if networks is None:
        check(L.aasr_run_stats_recipe(feat._h, gmm._h, topo.handle, recipe_path.encode(), C.byref(opts), C.byref(st)))
    else:
        check(L.aasr_run_stats_networks_recipe(feat._h, gmm._h, topo.handle, recipe_path.encode(), C.byref(opts),
                                               C.byref(networks), C.byref(st)))
    return {"utterances": st.utterances, "frames": st.frames, "seconds_total": st.seconds_total}


# ---- the log-likelihood of a state segmentation, VTLN estimation ---------------------------------

AASR_PHN_STATE_NUM_LABELS, AASR_PHN_RELATIVE_SAMPLES = 1, 2


class SegLL:
    """Owner of an aasr_segll handle: per frame safe_log(likelihood) of the one pdf its segmentation gives it -- the
    frame_ll of Stats.accumulate_dev from a kernel that sums nothing (any dimension, any mixture size)."""

    def __init__(self, gmm: "Gmm"):
        h = C.c_void_p()
        check(lib().aasr_segll_create(gmm._h, C.byref(h)))
        self._h = h.value

    def close(self) -> None:
        if self._h:
            lib().aasr_segll_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def score_dev(self, d_frames, pdf, d_frame_ll, stream=None) -> None:
        """d_frames: a float64 device tensor [n x dim]; pdf: host int32 per frame (-1: skip, its entry of d_frame_ll is
        left as it is); d_frame_ll: a float64 device tensor [n]."""
        p = np.ascontiguousarray(pdf, np.int32)
        check(lib().aasr_segll_score_dev(self._h, _ptr(d_frames), len(p), _ptr(p), _ptr(d_frame_ll),
                                         _stream_handle(stream)))

    def launch_shape(self) -> dict:
        """Diagnostic: the last score_dev call that launched the kernel (zeros before the first): work items, rows per LDS
        sub-block, a workgroup's LDS bytes, the doubles between two rows in LDS, the rows of the largest item."""
        out = (C.c_int32 * 5)()
        lib().aasr_debug_segll_shape(self._h, out)
        return {"items": int(out[0]), "sub": int(out[1]), "lds_bytes": int(out[2]), "stride": int(out[3]),
                "item_rows": int(out[4])}


def phn_read_segmentation(topo: Topology, path: str, frame_rate: float = 125.0, first_frame: int = 0,
                          last_frame: int = 0, eof_frame: int = -1, snl: bool = False, rsamp: bool = False,
                          transitions: bool = False):
    """stats_read_segmentation with PhnReader's two modes: state-number labels (snl) and sample numbers relative to the
    start time (rsamp).  Host only."""
    L = lib()
    sf, n = C.c_int32(), C.c_int32()
    pp, tp = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
    flags = (AASR_PHN_STATE_NUM_LABELS if snl else 0) | (AASR_PHN_RELATIVE_SAMPLES if rsamp else 0)
    check(L.aasr_phn_read_segmentation(topo.handle, path.encode(), frame_rate, first_frame, last_frame, eof_frame, flags,
                                       1 if transitions else 0, C.byref(sf), C.byref(pp), C.byref(tp), C.byref(n)))
    try:
        if n.value < 0:
            return None
        pdf = np.array([pp[k] for k in range(n.value)], np.int32)
        tr = np.array([tp[k] for k in range(n.value)], np.int32)
        return sf.value, pdf, tr
    finally:
        L.aasr_free(pp)
        L.aasr_free(tp)


# ---- HMM networks and the forward-backward pass ------------------------------------------------

FB_BAUM_WELCH, FB_VITERBI = 0, 1
FB_OK, FB_FAILED_BACKWARD, FB_FAILED_FORWARD = 1, 2, 3

_HMMNET_INT_ARRAYS = ("em_begin", "em_src", "em_tgt", "em_pdf", "em_tr", "em_self", "in_begin", "in_arcs", "pdfs",
                      "pdf_begin", "pdf_arcs", "trs", "tr_begin", "tr_arcs", "eo_begin", "ep_src", "ep_tgt", "ei_begin",
                      "ei_arcs", "bl_begin", "bl_nodes", "fl_begin", "fl_nodes")
_HMMNET_DOUBLE_ARRAYS = ("em_logp", "em_static", "ep_score")


class HmmNet:
    """Owner of an aasr_hmmnet handle: an HMM network file (HmmNetBaumWelch::read_fst) as the flat arrays the
    forward-backward kernel reads.  Host only."""

    def __init__(self, topo: Topology, path: str):
        h = C.c_void_p()
        check(lib().aasr_hmmnet_read(topo.handle, path.encode(), C.byref(h)))
        self._h = h.value

    def close(self) -> None:
        if self._h:
            lib().aasr_hmmnet_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self) -> int:
        return self._h

    def counts(self) -> dict:
        out = np.zeros(9, np.int32)
        check(lib().aasr_hmmnet_counts(self._h, _ptr(out)))
        names = ("nodes", "emitting", "epsilon", "backward_levels", "forward_levels", "pdfs", "transitions", "initial",
                 "final")
        return {k: int(v) for k, v in zip(names, out)}

    def array(self, name: str) -> np.ndarray:
        """One of the reader's arrays by its name in csrc/hmmnet.h."""
        if name in _HMMNET_INT_ARRAYS:
            which, dtype = _HMMNET_INT_ARRAYS.index(name), np.int32
        else:
            which, dtype = 100 + _HMMNET_DOUBLE_ARRAYS.index(name), np.float64
        n = C.c_int64()
        check(lib().aasr_hmmnet_array(self._h, which, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype)
        check(lib().aasr_hmmnet_array(self._h, which, _ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def arc_label(self, arc: int) -> Optional[str]:
        s = lib().aasr_hmmnet_arc_label(self._h, arc)
        return None if s is None else s.decode()


class FbOptions(C.Structure):
    """aasr_fb_options up to device_occ: the fields the struct had before want_path, under the name their callers
    know.  The library reads the whole struct, FbPathOptions below; defaults() returns that, and fb_batch /
    fb_batch_entries complete an instance of this class before they hand it on.
    Never pass C.byref(FbOptions()) to the library yourself: it reads want_path, 4 bytes past this class's end."""
    _fields_ = [("fw_beam", C.c_double), ("bw_beam", C.c_double), ("ac_scale", C.c_double), ("mode", C.c_int32),
                ("max_attempts", C.c_int32), ("want_pdf_occ", C.c_int32), ("want_tr_occ", C.c_int32),
                ("force_global", C.c_int32), ("device_occ", C.c_int32)]

    @classmethod
    def defaults(cls) -> "FbPathOptions":
        o = FbPathOptions()
        lib().aasr_fb_default_options(C.byref(o))
        return o


class FbPathOptions(FbOptions):
    """The whole aasr_fb_options: FbOptions and the struct's last field, want_path (a ctypes subclass appends its
    fields to its base's: want_path lies at offset 48, as in the header)."""
    _fields_ = [("want_path", C.c_int32)]


def _whole_fb_options(opts: Optional[FbOptions]) -> FbPathOptions:
    if opts is None:
        return FbOptions.defaults()
    if isinstance(opts, FbPathOptions):
        return opts
    o = FbPathOptions()
    for name, _ in FbOptions._fields_:
        setattr(o, name, getattr(opts, name))
    assert C.sizeof(o) == 56 and FbPathOptions.want_path.offset == 48      # sizeof(aasr_fb_options)
    return o


def fb_batch(nets: list, n_frames: list, scores, row0: list, opts: Optional[FbOptions] = None, stream: int = 0) -> list:
    """Forward-backward over HMM networks on the device.  nets[u]: the HmmNet of utterance u; scores: a device tensor
    of state log-likelihood rows (float32 or float64), row0[u] the row of utterance u's first frame.  Utterances whose
    backward pass misses the initial node are launched again with backward beam 2x, 3x, ... up to max_attempts.
    Returns per utterance a dict: status, backward_total, forward_total, attempts, pdf_occ, tr_occ (the last two None
    unless the options ask for them), and `shape`, the launch shape of the first attempt.  With opts.want_path also
    `path`, the emitting arc of every frame (int32), or for an utterance that did not run `path_refused`: the status
    and message with which aasr_fb_batch_path refused it."""
    L = lib()
    opts = _whole_fb_options(opts)
    n = len(nets)
    handles = (C.c_void_p * max(n, 1))(*[h.handle for h in nets])
    T = np.ascontiguousarray(n_frames, np.int32)
    r0 = np.ascontiguousarray(row0, np.int64)
    b = C.c_void_p()
    check(L.aasr_fb_batch_create(C.byref(opts), n, handles, _ptr(T), C.byref(b)))
    try:
        f64 = 1 if str(scores.dtype) == "torch.float64" else 0
        failed = C.c_int32(0)
        shape = None
        for attempt in range(1, opts.max_attempts + 1):
            check(L.aasr_fb_batch_dev(b, _ptr(scores), scores.shape[1], scores.shape[0], f64, _ptr(r0), attempt, stream))
            check(L.aasr_fb_batch_sync(b, stream, C.byref(failed)))
            if shape is None:
                sh = (C.c_int32 * 4)()
                L.aasr_debug_fb_shape(b, sh)
                shape = {"utterances": int(sh[0]), "lds_form": int(sh[1]), "lds_bytes": int(sh[2]), "attempt": int(sh[3])}
            if failed.value == 0:
                break
        out = []
        for u in range(n):
            c = nets[u].counts()
            st, at = C.c_int32(), C.c_int32()
            bt, ft = C.c_double(), C.c_double()
            occ = np.zeros((int(T[u]), c["pdfs"]), np.float64) if opts.want_pdf_occ else None
            trocc = np.zeros(c["transitions"], np.float64) if opts.want_tr_occ else None
            check(L.aasr_fb_batch_result(b, u, C.byref(st), C.byref(bt), C.byref(ft), C.byref(at), _ptr(occ), _ptr(trocc)))
            out.append({"status": st.value, "backward_total": bt.value, "forward_total": ft.value, "attempts": at.value,
                        "pdf_occ": occ, "tr_occ": trocc, "shape": shape, "device_bytes": L.aasr_fb_batch_device_bytes(b)})
            if opts.want_path:
                path = np.full(int(T[u]), -1, np.int32)
                rc = L.aasr_fb_batch_path(b, u, _ptr(path))
                if rc == 0:
                    out[-1]["path"] = path
                else:
                    out[-1]["path_refused"] = (int(rc), L.aasr_last_error().decode())
        return out
    finally:
        L.aasr_fb_batch_destroy(b)


def fb_batch_entries(nets: list, n_frames: list, scores, row0: list, n_states: int, opts: Optional[FbOptions] = None,
                     frame_row0: Optional[list] = None, stream: int = 0) -> dict:
    """The forward-backward pass of fb_batch with the occupancies kept on the device (device_occ) and turned into
    weighted statistics entries there (aasr_fb_batch_entries_dev).  frame_row0[u]: the frame row of utterance u's first
    frame in the entries (default: row0).  Returns status / forward_total / attempts per utterance, cnt (n_states + 1),
    rows and weights (copied to the host for the caller to look at), sums (per utterance that ran, its frame sums; None
    for the others), shape (aasr_debug_fb_entries_shape) and pdf_occ_refused: the message with which
    aasr_fb_batch_result refused the occupancies."""
    L = lib()
    o = _whole_fb_options(opts)
    o.want_pdf_occ = o.device_occ = 1
    n = len(nets)
    handles = (C.c_void_p * max(n, 1))(*[h.handle for h in nets])
    T = np.ascontiguousarray(n_frames, np.int32)
    r0 = np.ascontiguousarray(row0, np.int64)
    fr0 = np.ascontiguousarray(row0 if frame_row0 is None else frame_row0, np.int64)
    b = C.c_void_p()
    check(L.aasr_fb_batch_create(C.byref(o), n, handles, _ptr(T), C.byref(b)))
    try:
        f64 = 1 if str(scores.dtype) == "torch.float64" else 0
        failed = C.c_int32(0)
        for attempt in range(1, o.max_attempts + 1):
            check(L.aasr_fb_batch_dev(b, _ptr(scores), scores.shape[1], scores.shape[0], f64, _ptr(r0), attempt, stream))
            check(L.aasr_fb_batch_sync(b, stream, C.byref(failed)))
            if failed.value == 0:
                break
        out = {"status": [], "forward_total": [], "attempts": [], "sums": []}
        cnt = np.zeros(n_states + 1, np.int64)
        d_rows, d_w = C.c_void_p(), C.c_void_p()
        check(L.aasr_fb_batch_entries_dev(b, n_states, _ptr(fr0), stream, _ptr(cnt), C.byref(d_rows), C.byref(d_w)))
        total = int(cnt[-1])
        rows, weights = np.zeros(total, np.int32), np.zeros(total, np.float64)
        check(L.aasr_fb_batch_entries_host(b, _ptr(rows), _ptr(weights)))
        for u in range(n):
            st, at, ft = C.c_int32(), C.c_int32(), C.c_double()
            check(L.aasr_fb_batch_result(b, u, C.byref(st), None, C.byref(ft), C.byref(at), None, None))
            out["status"].append(st.value)
            out["forward_total"].append(ft.value)
            out["attempts"].append(at.value)
            if st.value == FB_OK:
                s = np.zeros(int(T[u]), np.float64)
                check(L.aasr_fb_batch_frame_sums(b, u, _ptr(s)))
                out["sums"].append(s)
            else:
                out["sums"].append(None)
        occ = np.zeros((int(T[0]), nets[0].counts()["pdfs"]), np.float64)
        rc = L.aasr_fb_batch_result(b, 0, None, None, None, None, _ptr(occ), None) if n else 0
        out["pdf_occ_refused"] = (int(rc), L.aasr_last_error().decode()) if rc != 0 else None
        sh = (C.c_int32 * 5)()
        L.aasr_debug_fb_entries_shape(b, sh)
        out["shape"] = {"entries": int(sh[0]), "utterances": int(sh[1]), "sum_groups": int(sh[2]), "count_groups": int(sh[3]),
                        "fill_groups": int(sh[4])}
        out.update(cnt=cnt, rows=rows, weights=weights)
        return out
    finally:
        L.aasr_fb_batch_destroy(b)


def fb_batch_frame_entries(nets: list, n_frames: list, scores, row0: list, n_states: int, opts: Optional[FbOptions] = None,
                           frame_row0: Optional[list] = None, n_rows: Optional[int] = None, stream: int = 0,
                           pdf_major: bool = False) -> dict:
    """fb_batch_entries' pass with the entries grouped by frame (aasr_fb_batch_frame_entries_dev): off (n_rows + 1), pdf
    and weight copied to the host, status / forward_total / attempts per utterance, sums (per utterance that ran, its
    frame sums, fetched after the frame-major call), shape (aasr_debug_fb_frame_entries_shape).  n_rows: the rows of the
    caller's frame buffer (default: the rows of `scores`).  pdf_major: also cnt / rows / weights of
    aasr_fb_batch_entries_dev on the same batch, taken first."""
    L = lib()
    o = _whole_fb_options(opts)
    o.want_pdf_occ = o.device_occ = 1
    n = len(nets)
    handles = (C.c_void_p * max(n, 1))(*[h.handle for h in nets])
    T = np.ascontiguousarray(n_frames, np.int32)
    r0 = np.ascontiguousarray(row0, np.int64)
    fr0 = np.ascontiguousarray(row0 if frame_row0 is None else frame_row0, np.int64)
    n_rows = int(scores.shape[0] if n_rows is None else n_rows)
    b = C.c_void_p()
    check(L.aasr_fb_batch_create(C.byref(o), n, handles, _ptr(T), C.byref(b)))
    try:
        f64 = 1 if str(scores.dtype) == "torch.float64" else 0
        failed = C.c_int32(0)
        for attempt in range(1, o.max_attempts + 1):
            check(L.aasr_fb_batch_dev(b, _ptr(scores), scores.shape[1], scores.shape[0], f64, _ptr(r0), attempt, stream))
            check(L.aasr_fb_batch_sync(b, stream, C.byref(failed)))
            if failed.value == 0:
                break
        out = {"status": [], "forward_total": [], "attempts": [], "sums": []}
        if pdf_major:
            cnt = np.zeros(n_states + 1, np.int64)
            d_rows, d_w = C.c_void_p(), C.c_void_p()
            check(L.aasr_fb_batch_entries_dev(b, n_states, _ptr(fr0), stream, _ptr(cnt), C.byref(d_rows), C.byref(d_w)))
            rows, weights = np.zeros(int(cnt[-1]), np.int32), np.zeros(int(cnt[-1]), np.float64)
            check(L.aasr_fb_batch_entries_host(b, _ptr(rows), _ptr(weights)))
            out.update(cnt=cnt, rows=rows, weights=weights)
        total = C.c_int64(0)
        d_off, d_pdf, d_w = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(L.aasr_fb_batch_frame_entries_dev(b, n_states, _ptr(fr0), n_rows, stream, C.byref(total), C.byref(d_off),
                                                C.byref(d_pdf), C.byref(d_w)))
        off = np.zeros(n_rows + 1, np.int64)
        pdf, weight = np.zeros(total.value, np.int32), np.zeros(total.value, np.float64)
        check(L.aasr_fb_batch_frame_entries_host(b, _ptr(off), _ptr(pdf), _ptr(weight)))
        for u in range(n):
            st, at, ft = C.c_int32(), C.c_int32(), C.c_double()
            check(L.aasr_fb_batch_result(b, u, C.byref(st), None, C.byref(ft), C.byref(at), None, None))
            out["status"].append(st.value)
            out["forward_total"].append(ft.value)
            out["attempts"].append(at.value)
            if st.value == FB_OK:
                s = np.zeros(int(T[u]), np.float64)
                check(L.aasr_fb_batch_frame_sums(b, u, _ptr(s)))
                out["sums"].append(s)
            else:
                out["sums"].append(None)
        sh = (C.c_int32 * 5)()
        L.aasr_debug_fb_frame_entries_shape(b, sh)
        out["shape"] = {"entries": int(sh[0]), "utterances": int(sh[1]), "count_groups": int(sh[2]), "scan_groups": int(sh[3]),
                        "fill_groups": int(sh[4])}
        out.update(n_entries=total.value, off=off, pdf=pdf, weight=weight)
        return out
    finally:
        L.aasr_fb_batch_destroy(b)


class LoglOptions(C.Structure):
    """aasr_logl_options: logl's options (aku/logl.cc:91-112)."""
    _fields_ = [("ophn", C.c_int32), ("snl", C.c_int32), ("hmmnet", C.c_int32), ("den_hmmnet", C.c_int32),
                ("mpv", C.c_int32), ("vit", C.c_int32), ("ac_scale_given", C.c_int32), ("info", C.c_int32),
                ("num_batches", C.c_int32), ("batch_index", C.c_int32), ("fw_beam", C.c_double), ("bw_beam", C.c_double),
                ("ac_scale", C.c_double), ("speakers", C.c_void_p)]

    @classmethod
    def defaults(cls, **kw) -> "LoglOptions":
        o = cls()
        lib().aasr_logl_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def run_logl_recipe(feat: "Feat", gmm: "Gmm", topo: Topology, recipe_path: str, opts: Optional[LoglOptions] = None,
                    speakers: Optional["SpeakerConfig"] = None) -> dict:
    """logl over a recipe -> the total log-likelihood (the per-file lines of info > 0 go to the process's stdout)"""
    opts = opts or LoglOptions.defaults()
    opts.speakers = speakers._h if speakers is not None else None
    st, total = RunStats(), C.c_double()
    check(lib().aasr_run_logl_recipe(feat._h, gmm._h, topo.handle, recipe_path.encode(), C.byref(opts), C.byref(total),
                                     C.byref(st)))
    return {"total": total.value, "utterances": st.utterances, "frames": st.frames, "seconds_total": st.seconds_total}


class VtlnOptions(C.Structure):
    """aasr_vtln_options: vtln's options (aku/vtln.cc:158-178)."""
    _fields_ = [("ophn", C.c_int32), ("snl", C.c_int32), ("rsamp", C.c_int32), ("info", C.c_int32),
                ("num_batches", C.c_int32), ("batch_index", C.c_int32), ("grid_size", C.c_int32),
                ("grid_size_given", C.c_int32), ("grid_rad", C.c_float), ("grid_rad_given", C.c_int32),
                ("relative", C.c_int32), ("module", C.c_char_p), ("speakers", C.c_void_p), ("out", C.c_char_p),
                ("savesum", C.c_char_p)]

    @classmethod
    def defaults(cls, **kw) -> "VtlnOptions":
        o = cls()
        lib().aasr_vtln_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def vtln_grid(opts: VtlnOptions):
    """(grid_start, grid_step, grid_size) of aku/vtln.cc:214-225 as float32 / int: the warp factor of grid point i is
    float32(centre + grid_start + i * grid_step)."""
    a, b, n = C.c_float(), C.c_float(), C.c_int32()
    lib().aasr_vtln_grid(C.byref(opts), C.byref(a), C.byref(b), C.byref(n))
    return np.float32(a.value), np.float32(b.value), int(n.value)


def vtln_summary_text(speakers, warps, logliks) -> str:
    """save_vtln_stats: speakers [ids], warps / logliks [per speaker a sequence] -> the summary file's text"""
    ids = [x.encode() for x in speakers]
    arr = (C.c_char_p * max(1, len(ids)))(*ids)
    counts = np.array([len(w) for w in warps], np.int32)
    w = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32) for x in warps] + [np.zeros(0, np.float32)]))
    ll = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float64) for x in logliks] + [np.zeros(0)]))
    text, n = C.c_void_p(), C.c_int64()
    check(lib().aasr_vtln_summary_text(arr, len(ids), _ptr(counts), _ptr(w), _ptr(ll), C.byref(text), C.byref(n)))
    try:
        return C.string_at(text.value, n.value).decode()
    finally:
        lib().aasr_free(text)


def vtln_set_group_frames(frames: int) -> None:
    """Diagnostic: the bound on a group's frames in run_vtln_recipe (<= 0: the default)."""
    lib().aasr_debug_vtln_set_group_frames(int(frames))


def run_vtln_recipe(feat: "Feat", gmm: "Gmm", topo: Topology, recipe_path: str, speakers: "SpeakerConfig", module: str,
                    out: Optional[str] = None, savesum: Optional[str] = None,
                    opts: Optional[VtlnOptions] = None) -> dict:
    opts = opts or VtlnOptions.defaults()
    ob, sb, mb = (out.encode() if out else None), (savesum.encode() if savesum else None), module.encode()
    opts.out, opts.savesum, opts.module, opts.speakers = ob, sb, mb, speakers._h
    st = RunStats()
    check(lib().aasr_run_vtln_recipe(feat._h, gmm._h, topo.handle, recipe_path.encode(), C.byref(opts), C.byref(st)))
    return {"utterances": st.utterances, "frames": st.frames, "seconds_total": st.seconds_total}


# ---- CMLLR estimation ---------------------------------------------------------------------------

class MllrOptions(C.Structure):
    """aasr_mllr_options: mllr's options (aku/mllr.cc:153-180) for global transforms over .phn files."""
    _fields_ = [("ophn", C.c_int32), ("info", C.c_int32), ("num_batches", C.c_int32), ("batch_index", C.c_int32),
                ("minframes", C.c_double), ("module", C.c_char_p), ("speakers", C.c_void_p), ("out", C.c_char_p)]

    @classmethod
    def defaults(cls, **kw) -> "MllrOptions":
        o = cls()
        lib().aasr_mllr_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


class Mllr:
    """Owner of an aasr_mllr handle: the CMLLR statistics G, k, beta of the current speaker, on the device."""

    def __init__(self, gmm: "Gmm"):
        h = C.c_void_p()
        check(lib().aasr_mllr_create(gmm._h, C.byref(h)))
        self._h = h.value
        self.D = gmm.dim

    def close(self) -> None:
        if self._h:
            lib().aasr_mllr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, stream=None) -> None:
        check(lib().aasr_mllr_reset(self._h, _stream_handle(stream)))

    def accumulate_dev(self, d_frames, pdf, stream=None) -> None:
        """d_frames: a float64 device tensor [n x dim]; pdf: host int32 per frame (-1: skip)."""
        p = np.ascontiguousarray(pdf, np.int32)
        check(lib().aasr_mllr_accumulate_dev(self._h, _ptr(d_frames), len(p), _ptr(p), _stream_handle(stream)))

    def accumulate_weighted_dev(self, d_frames, d_off, d_pdf, d_weight, stream=None) -> None:
        """d_frames: a float64 device tensor [n x dim]; d_off: an int64 device tensor [n + 1] of offsets into d_pdf (int32)
        and d_weight (float64), device tensors of the entries -- the layout of aasr_fb_batch_frame_entries_dev."""
        n, e = int(d_off.shape[0]) - 1, int(d_pdf.shape[0])
        assert n >= 0 and int(d_weight.shape[0]) == e and (n == 0 or int(d_frames.shape[0]) >= n)
        check(lib().aasr_mllr_accumulate_weighted_dev(self._h, _ptr(d_frames), n, _ptr(d_off), _ptr(d_pdf) if e else None,
                                                      _ptr(d_weight) if e else None, e, _stream_handle(stream)))

    def fetch(self, stream=None):
        """Waits for the device; -> G [dim][dim + 1][dim + 1], k [dim][dim + 1], beta."""
        L = lib()
        check(L.aasr_mllr_fetch(self._h, _stream_handle(stream)))
        D = self.D
        G, k, beta = np.zeros((D, D + 1, D + 1)), np.zeros((D, D + 1)), C.c_double()
        check(L.aasr_mllr_get(self._h, _ptr(G), _ptr(k), C.byref(beta)))
        return G, k, beta.value


def mllr_solve(G, k, beta: float):
    """MllTrainerComponent::calculate_transform (host only): W [dim][dim + 1], column 0 the bias."""
    G, k = np.ascontiguousarray(G, np.float64), np.ascontiguousarray(k, np.float64)
    D = k.shape[0]
    W = np.zeros((D, D + 1))
    check(lib().aasr_mllr_solve(D, _ptr(G), _ptr(k), float(beta), _ptr(W)))
    return W


def mllr_compose(W, old_A=None, old_b=None):
    """MllrTrainer::calculate_transform(LinTransformModule *) (host only): -> float32 A [dim x dim], b [dim]."""
    W = np.ascontiguousarray(W, np.float64)
    D = W.shape[0]
    A, b = np.zeros((D, D), np.float32), np.zeros(D, np.float32)
    oa = np.ascontiguousarray(old_A, np.float32) if old_A is not None else None
    ob = np.ascontiguousarray(old_b, np.float32) if old_b is not None else None
    check(lib().aasr_mllr_compose(D, _ptr(W), _ptr(oa), _ptr(ob), _ptr(A), _ptr(b)))
    return A, b


class MllrNetworkOptions(C.Structure):
    """aasr_mllr_network_options: what mllr --networks adds (--segmode vit, -F, -W)."""
    _fields_ = [("networks", C.c_int32), ("viterbi", C.c_int32), ("fw_beam", C.c_double), ("bw_beam", C.c_double)]

    @classmethod
    def defaults(cls, **kw) -> "MllrNetworkOptions":
        o = cls()
        lib().aasr_mllr_network_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def run_mllr_recipe(feat: "Feat", gmm: "Gmm", topo: Topology, recipe_path: str, speakers: SpeakerConfig,
                    out: Optional[str] = None, module: Optional[str] = None,
                    opts: Optional[MllrOptions] = None, networks: Optional[MllrNetworkOptions] = None) -> dict:
    """mllr over a recipe; with `networks` (its networks field set) over the recipe's hmmnet= networks (mllr --networks)"""
    opts = opts or MllrOptions.defaults()
    ob, mb = (out.encode() if out else None), (module.encode() if module else None)
    opts.out, opts.module, opts.speakers = ob, mb, speakers._h
    st = RunStats()
    if networks is None:
        check(lib().aasr_run_mllr_recipe(feat._h, gmm._h, topo.handle, recipe_path.encode(), C.byref(opts), C.byref(st)))
    else:
        check(lib().aasr_run_mllr_networks_recipe(feat._h, gmm._h, topo.handle, recipe_path.encode(), C.byref(opts),
                                                  C.byref(networks), C.byref(st)))
    return {"utterances": st.utterances, "frames": st.frames, "seconds_total": st.seconds_total}


# ---- LDA estimation -----------------------------------------------------------------------------

class Scatter:
    """Owner of an aasr_scatter handle: per class gamma, sum gamma x and sum gamma x x^T, on the device."""

    def __init__(self, n_classes: int, dim: int):
        h = C.c_void_p()
        check(lib().aasr_scatter_create(n_classes, dim, C.byref(h)))
        self._h = h.value
        self.C, self.D = n_classes, dim

    def close(self) -> None:
        if self._h:
            lib().aasr_scatter_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def accumulate_dev(self, d_frames, cls, d_weight=None, stream=None) -> None:
        """d_frames: a float64 device tensor [n x dim]; cls: host int32 per frame (-1: skip); d_weight: a float64
        device tensor [n] or None (1)."""
        c = np.ascontiguousarray(cls, np.int32)
        check(lib().aasr_scatter_accumulate_dev(self._h, _ptr(d_frames), len(c), _ptr(c), _ptr(d_weight),
                                                _stream_handle(stream)))

    def accumulate_weighted_dev(self, d_frames, cnt, d_rows, d_weights, stream=None) -> None:
        """Weighted entries, class run after class run: cnt host int64 [C + 1] (cnt[c]: the first entry of class c);
        d_rows: an int32 device tensor of frame rows, d_weights: a float64 device tensor, cnt[C] elements each (None
        passes a null array).  A frame may stand under several classes; an entry of weight 0 does not read its row."""
        c = np.ascontiguousarray(cnt, np.int64)
        if len(c) != self.C + 1:
            raise ValueError("cnt must hold n_classes + 1 values")
        n = int(d_frames.shape[0]) if d_frames is not None else 0
        check(lib().aasr_scatter_accumulate_weighted_dev(self._h, _ptr(d_frames), n, _ptr(c), _ptr(d_rows), _ptr(d_weights),
                                                         _stream_handle(stream)))

    def set_slab_bytes(self, nbytes: int) -> None:
        """Diagnostic: the bound on a launch's slab memory."""
        check(lib().aasr_debug_scatter_set_slab_bytes(self._h, nbytes))

    def launch_shape(self) -> dict:
        """Diagnostic: the kernel instance, the work items and the launches of the last call that added rows."""
        out = (C.c_int32 * 3)()
        lib().aasr_debug_scatter_shape(self._h, out)
        return {"pb": int(out[0]), "items": int(out[1]), "launches": int(out[2])}

    def fetch(self, stream=None):
        """Waits for the device; -> gamma [C], sum_x [C x dim], sum_xx [C x dim (dim + 1) / 2] (packed lower
        triangle, row-major with j <= i)."""
        L = lib()
        check(L.aasr_scatter_fetch(self._h, _stream_handle(stream)))
        g, sx = np.zeros(self.C), np.zeros((self.C, self.D))
        sxx = np.zeros((self.C, self.D * (self.D + 1) // 2))
        check(L.aasr_scatter_get(self._h, _ptr(g), _ptr(sx), _ptr(sxx)))
        return g, sx, sxx


def lda_solve(gamma, sum_x, sum_xx, selected, max_gamma: float, target_dim: int):
    """lda.cc:380-446 (host only): -> lda [target_dim x dim]; rows by falling eigenvalue of the projected covariance,
    every row's largest-magnitude entry positive."""
    g, sx = np.ascontiguousarray(gamma, np.float64), np.ascontiguousarray(sum_x, np.float64)
    sxx, sel = np.ascontiguousarray(sum_xx, np.float64), np.ascontiguousarray(selected, np.int32)
    n, D = sx.shape
    out = np.zeros((target_dim, D))
    check(lib().aasr_lda_solve(n, D, _ptr(g), _ptr(sx), _ptr(sxx), _ptr(sel), float(max_gamma), target_dim, _ptr(out)))
    return out


def lda_select(count, mingamma: float, maxmem: int, dim: int, silence=()):
    """lda.cc:113-115, 247-263 (host only): -> 0 / 1 per state."""
    c = np.ascontiguousarray(count, np.float64)
    sil = np.ascontiguousarray(silence, np.int32)
    out = np.zeros(len(c), np.int32)
    check(lib().aasr_lda_select(len(c), _ptr(c), float(mingamma), maxmem, dim, _ptr(sil) if len(sil) else None, len(sil),
                                _ptr(out)))
    return out


class LdaOptions(C.Structure):
    """aasr_lda_options: lda's options (aku/lda.cc:51-72) over .phn files."""
    _fields_ = [("ophn", C.c_int32), ("info", C.c_int32), ("target_dim", C.c_int32), ("maxmem", C.c_int32),
                ("no_silence", C.c_int32), ("mingamma", C.c_double), ("maxgamma", C.c_double), ("module", C.c_char_p),
                ("speakers", C.c_char_p), ("out", C.c_char_p), ("state_gamma", C.c_void_p),
                ("seconds_scatter", C.c_double), ("seconds_features", C.c_double)]

    @classmethod
    def defaults(cls, **kw) -> "LdaOptions":
        o = cls()
        lib().aasr_lda_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def run_lda_recipe(cfg_text: str, topo: Topology, recipe_path: str, module: str, target_dim: int,
                   out: Optional[str] = None, speakers: Optional[str] = None, opts: Optional[LdaOptions] = None) -> dict:
    """-> the run's counts and device times, and "state_gamma": the scatter handle's gamma of every state."""
    opts = opts or LdaOptions.defaults()
    mb, ob, sb = module.encode(), (out.encode() if out else None), (speakers.encode() if speakers else None)
    opts.module, opts.out, opts.speakers, opts.target_dim = mb, ob, sb, target_dim
    sg = np.zeros(topo.num_states())
    opts.state_gamma = sg.ctypes.data
    st = RunStats()
    check(lib().aasr_run_lda_recipe(cfg_text.encode(), topo.handle, recipe_path.encode(), C.byref(opts), C.byref(st)))
    return {"utterances": st.utterances, "frames": st.frames, "seconds_total": st.seconds_total,
            "seconds_scatter": opts.seconds_scatter, "seconds_features": opts.seconds_features, "state_gamma": sg}


class LdaNetworkOptions(C.Structure):
    """aasr_lda_network_options: what lda --networks adds (--segmode vit, -F, -W, -A)."""
    _fields_ = [("networks", C.c_int32), ("viterbi", C.c_int32), ("fw_beam", C.c_double), ("bw_beam", C.c_double),
                ("ac_scale_given", C.c_int32), ("ac_scale", C.c_double)]

    @classmethod
    def defaults(cls, **kw) -> "LdaNetworkOptions":
        o = cls()
        lib().aasr_lda_network_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def run_lda_networks_recipe(cfg_text: str, gmm: "Gmm", topo: Topology, recipe_path: str, module: str, target_dim: int,
                            out: Optional[str] = None, speakers: Optional[str] = None, opts: Optional[LdaOptions] = None,
                            networks: Optional[LdaNetworkOptions] = None) -> dict:
    """lda over the recipe's hmmnet= networks (lda --networks); `networks` None: Baum-Welch with the default beams.
    -> as run_lda_recipe; "state_gamma" holds every state's summed posterior."""
    opts = opts or LdaOptions.defaults()
    networks = networks or LdaNetworkOptions.defaults(networks=1)
    mb, ob, sb = module.encode(), (out.encode() if out else None), (speakers.encode() if speakers else None)
    opts.module, opts.out, opts.speakers, opts.target_dim = mb, ob, sb, target_dim
    sg = np.zeros(topo.num_states())
    opts.state_gamma = sg.ctypes.data
    st = RunStats()
    check(lib().aasr_run_lda_networks_recipe(cfg_text.encode(), gmm._h if gmm is not None else None, topo.handle,
                                             recipe_path.encode(), C.byref(opts), C.byref(networks), C.byref(st)))
    return {"utterances": st.utterances, "frames": st.frames, "seconds_total": st.seconds_total,
            "seconds_scatter": opts.seconds_scatter, "seconds_features": opts.seconds_features, "state_gamma": sg}


# ---- Gaussian-pool clustering -------------------------------------------------------------------

def gcluster_chunk() -> int:
    """Diagnostic: the centres the assignment kernel walks at a time."""
    return int(lib().aasr_debug_gcluster_chunk())


def gcluster_assign(mean, cov, ldet, c_mean, c_cov, c_ldet, c_valid, euclid: bool = False):
    """One assignment pass of gcluster on the device: -> (index [G] int32, distance [G]).  euclid: the norm of the mean
    difference over all centres (only mean and c_mean are read); otherwise the Kullback-Leibler divergence over the
    centres with c_valid != 0."""
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
    mean, cov, ldet, c_mean, c_cov, c_ldet = f64(mean), f64(cov), f64(ldet), f64(c_mean), f64(c_cov), f64(c_ldet)
    c_valid = None if c_valid is None else np.ascontiguousarray(c_valid, np.int32)
    G, D = mean.shape
    Cn = c_mean.shape[0]
    if c_mean.shape[1] != D:
        raise ValueError("centres of %d dimensions for Gaussians of %d" % (c_mean.shape[1], D))
    idx, dist = np.zeros(G, np.int32), np.zeros(G)
    check(lib().aasr_gcluster_assign(D, G, _ptr(mean), _ptr(cov), _ptr(ldet), Cn, _ptr(c_mean), _ptr(c_cov), _ptr(c_ldet),
                                     _ptr(c_valid), 1 if euclid else 0, _ptr(idx), _ptr(dist)))
    return idx, dist


def gcluster_centres(mean, cov, cluster_map, n_clusters: int):
    """compute_cluster_statistics on the device: -> (c_mean, c_cov [C x D], c_ldet [C], c_valid [C] int32)."""
    mean, cov = np.ascontiguousarray(mean, np.float64), np.ascontiguousarray(cov, np.float64)
    m = np.ascontiguousarray(cluster_map, np.int32)
    G, D = mean.shape
    if len(m) != G or cov.shape != mean.shape:
        raise ValueError("mean, cov and the map disagree in shape")
    cm, cc = np.zeros((n_clusters, D)), np.zeros((n_clusters, D))
    cl, cv = np.zeros(n_clusters), np.zeros(n_clusters, np.int32)
    check(lib().aasr_gcluster_centres(D, G, _ptr(mean), _ptr(cov), n_clusters, _ptr(m), _ptr(cm), _ptr(cc), _ptr(cl), _ptr(cv)))
    return cm, cc, cl, cv


class GclusterOptions(C.Structure):
    """aasr_gcluster_options: gcluster's options (aku/gcluster.cc:359-369)."""
    _fields_ = [("clusters", C.c_int32), ("iterations", C.c_int32), ("info", C.c_int32), ("full", C.c_int32),
                ("progress", C.c_int32), ("regtree", C.c_char_p), ("base", C.c_char_p), ("written", C.c_int32),
                ("seconds_steps", C.c_double)]

    @classmethod
    def defaults(cls, **kw) -> "GclusterOptions":
        o = cls()
        lib().aasr_gcluster_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def gcluster(gk_path: str, out_path: str, clusters: int = 1000, info: int = 0, opts: Optional[GclusterOptions] = None) -> dict:
    """The gcluster tool's run: reads the .gk, writes the .gcl; -> the clusters written and the steps' time."""
    opts = opts or GclusterOptions.defaults()
    opts.clusters, opts.info = clusters, info
    check(lib().aasr_run_gcluster(gk_path.encode(), out_path.encode(), C.byref(opts)))
    return {"written": int(opts.written), "seconds_steps": float(opts.seconds_steps)}


def gcluster_arrays(mean, cov, clusters: int = 1000, info: int = 0):
    """The same run on arrays: -> (cluster of every Gaussian [G] int32, renumbered; clusters written; steps' seconds)."""
    mean, cov = np.ascontiguousarray(mean, np.float64), np.ascontiguousarray(cov, np.float64)
    G, D = mean.shape
    opts = GclusterOptions.defaults(clusters=clusters, info=info)
    out = np.zeros(G, np.int32)
    check(lib().aasr_gcluster_arrays(D, G, _ptr(mean), _ptr(cov), C.byref(opts), _ptr(out)))
    return out, int(opts.written), float(opts.seconds_steps)


# ---- feature normalization and PCA ---------------------------------------------------------------

MOMENTS_DIAG, MOMENTS_FULL = 0, 1


class Moments:
    """Owner of an aasr_moments handle: per segment (a contiguous run of frame rows) the count, sum x and sum x^2
    (MOMENTS_DIAG) or sum x x^T (MOMENTS_FULL), on the device."""

    def __init__(self, dim: int, mode: int = MOMENTS_DIAG):
        h = C.c_void_p()
        check(lib().aasr_moments_create(dim, mode, C.byref(h)))
        self._h = h.value
        self.D, self.full = dim, mode == MOMENTS_FULL

    def close(self) -> None:
        if self._h:
            lib().aasr_moments_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def accumulate_dev(self, d_frames, segments, stream=None) -> None:
        """d_frames: a float64 device tensor [n x dim]; segments: host int32 [m x 3] = first row, length, utterance."""
        s = np.ascontiguousarray(segments, np.int32).reshape(-1, 3)
        check(lib().aasr_moments_accumulate_dev(self._h, _ptr(d_frames), int(d_frames.shape[0]), _ptr(s), len(s),
                                                _stream_handle(stream)))

    def set_launch_segments(self, n: int) -> None:
        """Diagnostic: at most n segments a launch."""
        check(lib().aasr_debug_moments_set_launch_segments(self._h, n))

    def launch_shape(self) -> dict:
        """Diagnostic: the full-mode kernel's instance, the work items and the launches of the last call."""
        out = (C.c_int32 * 3)()
        lib().aasr_debug_moments_shape(self._h, out)
        return {"pb": int(out[0]), "items": int(out[1]), "launches": int(out[2])}

    def _xx(self) -> int:
        return self.D * (self.D + 1) // 2 if self.full else self.D

    def fetch(self, stream=None):
        """Waits for the device; per segment in the order given -> count [n], utterance [n], sum_x [n x dim], sum_xx
        ([n x dim] sum x^2, or [n x dim (dim + 1) / 2] the packed lower triangle of sum x x^T)."""
        L = lib()
        check(L.aasr_moments_fetch(self._h, _stream_handle(stream)))
        n = int(L.aasr_moments_num_segments(self._h))
        c, u = np.zeros(n), np.zeros(n, np.int32)
        sx, sxx = np.zeros((n, self.D)), np.zeros((n, self._xx()))
        check(L.aasr_moments_get(self._h, _ptr(c), _ptr(u), _ptr(sx), _ptr(sxx)))
        return c, u, sx, sxx

    def blocked(self, block_size: int, keep=None):
        """After a fetch: feanorm's blocked sums over the segments (keep [n]: 0 leaves one out) -> count, sum_x [dim],
        sum_xx."""
        k = None if keep is None else np.ascontiguousarray(keep, np.int32)
        c, sx, sxx = C.c_double(), np.zeros(self.D), np.zeros(self._xx())
        check(lib().aasr_moments_blocked(self._h, block_size, _ptr(k), C.byref(c), _ptr(sx), _ptr(sxx)))
        return c.value, sx, sxx


def feanorm_pca(cov, scale=None, unit_determinant: bool = False):
    """feanorm.cc:281-325 (host only): -> (pca [dim x dim], eigenvalues [dim] ascending); rows by ascending eigenvalue,
    every row's largest-magnitude entry positive."""
    cov = np.ascontiguousarray(cov, np.float64)
    d = cov.shape[0]
    sc = None if scale is None else np.ascontiguousarray(scale, np.float64)
    out, ev = np.zeros((d, d)), np.zeros(d)
    check(lib().aasr_feanorm_pca(d, _ptr(cov), _ptr(sc), 1 if unit_determinant else 0, _ptr(out), _ptr(ev)))
    return out, ev


class FeanormOptions(C.Structure):
    """aasr_feanorm_options: feanorm's options (aku/feanorm.cc:48-62)."""
    _fields_ = [("info", C.c_int32), ("block_size", C.c_int32), ("cov", C.c_int32), ("print", C.c_int32),
                ("unit_determinant", C.c_int32), ("module", C.c_char_p), ("pca", C.c_char_p), ("speakers", C.c_char_p),
                ("utt", C.c_char_p), ("out", C.c_char_p), ("blocks", C.c_double), ("seconds_moments", C.c_double),
                ("seconds_features", C.c_double)]

    @classmethod
    def defaults(cls, **kw) -> "FeanormOptions":
        o = cls()
        lib().aasr_feanorm_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def run_feanorm_recipe(cfg_text: str, recipe_path: str, module: Optional[str] = None, pca: Optional[str] = None,
                       out: Optional[str] = None, speakers: Optional[str] = None, utt: Optional[str] = None,
                       opts: Optional[FeanormOptions] = None) -> dict:
    """-> the run's counts, the global block count and the device times."""
    opts = opts or FeanormOptions.defaults()
    enc = lambda s: s.encode() if s else None
    opts.module, opts.pca, opts.out, opts.speakers, opts.utt = enc(module), enc(pca), enc(out), enc(speakers), enc(utt)
    st = RunStats()
    check(lib().aasr_run_feanorm_recipe(cfg_text.encode(), recipe_path.encode(), C.byref(opts), C.byref(st)))
    return {"utterances": st.utterances, "frames": st.frames, "seconds_total": st.seconds_total, "blocks": opts.blocks,
            "seconds_moments": opts.seconds_moments, "seconds_features": opts.seconds_features}


# ---- model re-estimation from statistics dumps ---------------------------------------------------


class Estimate:
    """Owner of an aasr_estimate handle (host only): a model's files with the accumulators that the dumps of stats are
    added to, the ML update, the pool edits and the writers of aku/estimate.cc."""

    def __init__(self, gk: str, mc: str, ph: str):
        h = C.c_void_p()
        check(lib().aasr_estimate_create(gk.encode(), mc.encode(), ph.encode(), C.byref(h)))
        self._h = h.value

    @classmethod
    def from_base(cls, base: str) -> "Estimate":
        return cls(base + ".gk", base + ".mc", base + ".ph")

    def close(self) -> None:
        if self._h:
            lib().aasr_estimate_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sizes(self) -> dict:
        out = (C.c_int32 * 7)()
        lib().aasr_estimate_sizes(self._h, out)
        return dict(zip(("gaussians", "dim", "mixtures", "components", "states", "transitions", "mode"), map(int, out)))

    def add_dump(self, base: str, transitions: bool = False) -> None:
        check(lib().aasr_estimate_add_dump(self._h, base.encode(), 1 if transitions else 0))

    def set_gaussian_parameters(self, minvar: float = 0.1, covsmooth: float = 0.0) -> None:
        check(lib().aasr_estimate_set_gaussian_parameters(self._h, float(minvar), float(covsmooth)))

    def estimate_transitions(self) -> None:
        check(lib().aasr_estimate_transitions(self._h))

    def estimate_ml(self, pool: bool = True, mixtures: bool = True) -> None:
        check(lib().aasr_estimate_ml(self._h, 1 if pool else 0, 1 if mixtures else 0))

    def delete_gaussians(self, minocc: float):
        """-> (index map of the pool before the call, Gaussians deleted)"""
        m, n = np.zeros(self.sizes()["gaussians"], np.int32), C.c_int32()
        check(lib().aasr_estimate_delete_gaussians(self._h, float(minocc), _ptr(m), C.byref(n)))
        return m, n.value

    def remove_mixture_components(self, min_weight: float):
        """-> (index map of the pool before the call, Gaussians deleted)"""
        m, n = np.zeros(self.sizes()["gaussians"], np.int32), C.c_int32()
        check(lib().aasr_estimate_remove_mixture_components(self._h, float(min_weight), _ptr(m), C.byref(n)))
        return m, n.value

    def split_gaussians(self, minocc: float = 0.0, maxmixgauss: int = 0, numgauss: int = -1, splitalpha: float = 1.0) -> int:
        n = C.c_int32()
        check(lib().aasr_estimate_split_gaussians(self._h, float(minocc), maxmixgauss, numgauss, float(splitalpha), C.byref(n)))
        return n.value

    def write(self, base: str) -> None:
        L = lib()
        check(L.aasr_estimate_write_mc(self._h, (base + ".mc").encode()))
        check(L.aasr_estimate_write_ph(self._h, (base + ".ph").encode()))
        check(L.aasr_estimate_write_gk(self._h, (base + ".gk").encode()))

    def statistics(self) -> dict:
        """The accumulated statistics in double (sum_xx: [G x dim], or the packed lower triangles in mode 3)."""
        z, L = self.sizes(), lib()
        G, D, M, K, T = z["gaussians"], z["dim"], z["mixtures"], z["components"], z["transitions"]
        xx = D * (D + 1) // 2 if z["mode"] & 2 else D
        acc, fc, g = np.zeros(G, np.int32), np.zeros(G, np.int32), np.zeros(G)
        sx, sxx = np.zeros((G, D)), np.zeros((G, xx))
        check(L.aasr_estimate_get_statistics(self._h, _ptr(acc), _ptr(fc), _ptr(g), _ptr(sx), _ptr(sxx)))
        macc, moff, mg = np.zeros(M, np.int32), np.zeros(M + 1, np.int32), np.zeros(K)
        check(L.aasr_estimate_get_mixture_statistics(self._h, _ptr(macc), _ptr(moff), _ptr(mg)))
        tacc, tocc = np.zeros(T, np.int32), np.zeros(T)
        check(L.aasr_estimate_get_transition_statistics(self._h, _ptr(tacc), _ptr(tocc)))
        return {"mode": z["mode"], "accumulated": acc, "feacount": fc, "gamma": g, "sum_x": sx, "sum_xx": sxx,
                "mix_accumulated": macc, "mix_offsets": moff, "mix_gamma": mg, "trans_accumulated": tacc, "trans_occ": tocc}

    def parameters(self) -> dict:
        """The current parameters in double."""
        z, L = self.sizes(), lib()
        G, D, M, K, T = z["gaussians"], z["dim"], z["mixtures"], z["components"], z["transitions"]
        mean, var = np.zeros((G, D)), np.zeros((G, D))
        check(L.aasr_estimate_get_gaussians(self._h, _ptr(mean), _ptr(var)))
        off, idx, w = np.zeros(M + 1, np.int32), np.zeros(K, np.int32), np.zeros(K)
        check(L.aasr_estimate_get_mixtures(self._h, _ptr(off), _ptr(idx), _ptr(w)))
        src, tgt, prob = np.zeros(T, np.int32), np.zeros(T, np.int32), np.zeros(T)
        check(L.aasr_estimate_get_transitions(self._h, _ptr(src), _ptr(tgt), _ptr(prob)))
        return {"mean": mean, "var": var, "mix_offsets": off, "mix_index": idx, "mix_weight": w, "trans_source": src,
                "trans_target": tgt, "trans_prob": prob}

    def run_mllt(self, old_matrix=None):
        """estimate --mllt over the handle's mode-3 statistics (device) -> A old_matrix in float32 [dim x dim]."""
        D = self.sizes()["dim"]
        old = None if old_matrix is None else np.ascontiguousarray(old_matrix, np.float32)
        out = np.zeros((D, D), np.float32)
        check(lib().aasr_estimate_run_mllt(self._h, _ptr(old), _ptr(out), None))
        return out


class Mllt:
    """Owner of an aasr_mllt handle: the Gaussians' covariances resident on the device, the variance and G passes of
    HmmSet::estimate_mllt over them."""

    def __init__(self, gamma, sum_x, sum_xx, accumulated=None):
        g = np.ascontiguousarray(gamma, np.float64)
        sx = np.ascontiguousarray(sum_x, np.float64).reshape(len(g), -1)
        self.G, self.D = sx.shape
        self.E = self.D * (self.D + 1) // 2
        sxx = np.ascontiguousarray(sum_xx, np.float64).reshape(self.G, -1)
        if sxx.shape[1] != self.E:
            raise ValueError("sum_xx must hold packed lower triangles [G x dim (dim + 1) / 2]")
        acc = None if accumulated is None else np.ascontiguousarray(accumulated, np.int32)
        h = C.c_void_p()
        check(lib().aasr_mllt_create(self.D, self.G, _ptr(g), _ptr(sx), _ptr(sxx), _ptr(acc), C.byref(h)))
        self._h = h.value

    def close(self) -> None:
        if self._h:
            lib().aasr_mllt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def covariances(self):
        out = np.zeros((self.G, self.E))
        check(lib().aasr_mllt_get_covariances(self._h, _ptr(out)))
        return out

    def variances(self, A):
        A = np.ascontiguousarray(A, np.float64)
        out = np.zeros((self.G, self.D))
        check(lib().aasr_mllt_variances(self._h, _ptr(A), _ptr(out)))
        return out

    def g_sums(self, var):
        """-> [dim x dim (dim + 1) / 2]: the packed lower triangle of sum_g (gamma_g / var_gi) S_g per dimension i."""
        v = np.ascontiguousarray(var, np.float64)
        out = np.zeros((self.D, self.E))
        check(lib().aasr_mllt_g_sums(self._h, _ptr(v), _ptr(out)))
        return out

    def estimate(self, minvar: float = 0.1):
        """The whole loop -> (A [dim x dim], mean [G x dim], var [G x dim]); rows of skipped Gaussians are zero."""
        A, mean, var = np.zeros((self.D, self.D)), np.zeros((self.G, self.D)), np.zeros((self.G, self.D))
        check(lib().aasr_mllt_estimate(self._h, float(minvar), _ptr(A), _ptr(mean), _ptr(var)))
        return A, mean, var

    def set_slab_bytes(self, nbytes: int) -> None:
        """Diagnostic: the bound on a launch's slab memory."""
        check(lib().aasr_debug_mllt_set_slab_bytes(self._h, nbytes))

    def launch_shape(self) -> dict:
        out = (C.c_int32 * 3)()
        lib().aasr_debug_mllt_shape(self._h, out)
        return {"pb": int(out[0]), "items": int(out[1]), "launches": int(out[2])}

    def times(self) -> dict:
        out = (C.c_double * 4)()
        lib().aasr_debug_mllt_times(self._h, out)
        return dict(zip(("cov_build", "variances", "g_sums", "host_solve"), map(float, out)))


def mllt_update_rows(A, g_inv, beta: float, iterations: int = 1):
    """aku/HmmSet.cc:955-980 (host only): `iterations` inner updates of A from the inverted G_i [dim x dim x dim]."""
    A = np.array(A, np.float64, order="C")
    gi = np.ascontiguousarray(g_inv, np.float64)
    check(lib().aasr_mllt_update_rows(A.shape[0], _ptr(gi), float(beta), iterations, _ptr(A)))
    return A


class EstimateOptions(C.Structure):
    """aasr_estimate_options: estimate's options (aku/estimate.cc:115-155) for --ml."""
    _fields_ = [("gk", C.c_char_p), ("mc", C.c_char_p), ("ph", C.c_char_p), ("base_name", C.c_char_p),
                ("config", C.c_char_p), ("list", C.c_char_p), ("out", C.c_char_p), ("mllt", C.c_char_p),
                ("savesum", C.c_char_p), ("transitions", C.c_int32), ("info", C.c_int32), ("minvar", C.c_double),
                ("covsmooth", C.c_double), ("delete_set", C.c_int32), ("delete_minocc", C.c_double),
                ("mremove_set", C.c_int32), ("mremove", C.c_double), ("split", C.c_int32), ("minocc_set", C.c_int32),
                ("minocc", C.c_double), ("maxmixgauss", C.c_int32), ("numgauss_set", C.c_int32), ("numgauss", C.c_int32),
                ("splitalpha", C.c_double), ("no_mixture_update", C.c_int32), ("no_write", C.c_int32),
                ("n_deleted", C.c_int32), ("n_removed", C.c_int32), ("n_splits", C.c_int32), ("seconds_read", C.c_double),
                ("seconds_mllt", C.c_double), ("seconds_mllt_parts", C.c_double * 4)]

    @classmethod
    def defaults(cls, **kw) -> "EstimateOptions":
        o = cls()
        lib().aasr_estimate_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def run_estimate(base: str, list_path: str, out: str, config: Optional[str] = None, mllt: Optional[str] = None,
                 savesum: Optional[str] = None, opts: Optional[EstimateOptions] = None) -> dict:
    """estimate --ml -b base -L list_path -o out [-c config] [--mllt MODULE] [-s savesum] -> the run's counts and times."""
    opts = opts or EstimateOptions.defaults()
    enc = lambda s: s.encode() if s else None
    opts.gk, opts.mc, opts.ph, opts.base_name = enc(base + ".gk"), enc(base + ".mc"), enc(base + ".ph"), enc(base)
    opts.config, opts.list, opts.out, opts.mllt, opts.savesum = enc(config), enc(list_path), enc(out), enc(mllt), enc(savesum)
    check(lib().aasr_run_estimate(C.byref(opts)))
    return {"n_deleted": opts.n_deleted, "n_removed": opts.n_removed, "n_splits": opts.n_splits,
            "seconds_read": opts.seconds_read, "seconds_mllt": opts.seconds_mllt,
            "seconds_mllt_parts": list(opts.seconds_mllt_parts)}


# ---- decision-tree state tying ------------------------------------------------------------------

def _take_text(call) -> bytes:
    out, n = C.c_void_p(), C.c_int64()
    check(call(C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value)
    finally:
        lib().aasr_free(out)


def tie_parse_label(label: str):
    """PhonePool's label functions (host only): -> (centre, left contexts, right contexts), nearest first."""
    c, l, r = _take_text(lambda o, n: lib().aasr_tie_parse_label(label.encode("latin-1"), o, n)).decode("latin-1").split("\n")
    return c, (l.split("\x1f") if l else []), (r.split("\x1f") if r else [])


class TieOptions(C.Structure):
    """aasr_tie_options: tie's options (aku/tie.cc:115-136) over .phn files."""
    _fields_ = [("ophn", C.c_int32), ("hmmnet", C.c_int32), ("info", C.c_int32), ("count", C.c_int32),
                ("context", C.c_int32), ("mloss_given", C.c_int32), ("hops", C.c_int32), ("clusters", C.c_int32),
                ("sgain", C.c_double), ("mloss", C.c_double), ("rule", C.c_char_p), ("speakers", C.c_char_p),
                ("out", C.c_char_p), ("basebind", C.c_char_p), ("seconds_scatter", C.c_double),
                ("seconds_features", C.c_double), ("seconds_split", C.c_double), ("seconds_merge", C.c_double)]

    @classmethod
    def defaults(cls, **kw) -> "TieOptions":
        o = cls()
        lib().aasr_tie_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


class Tie:
    """Owner of an aasr_tie handle: rules, context phones, their statistics on the device, the trees."""

    def __init__(self, dim: int, rule_path: str):
        h = C.c_void_p()
        check(lib().aasr_tie_create(dim, rule_path.encode(), C.byref(h)))
        self._h = h.value
        self.D = dim
        self.E = 1 + dim + dim * (dim + 1) // 2

    def close(self) -> None:
        if self._h:
            lib().aasr_tie_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rules(self):
        """[(name, [phones in set order])]"""
        t = _take_text(lambda o, n: lib().aasr_tie_rules_text(self._h, o, n)).decode("latin-1")
        return [(f[0], f[1:]) for f in (line.split("\x1f") for line in t.split("\n")[:-1])]

    def context_phone(self, label: str, state: int) -> int:
        c = C.c_int32()
        check(lib().aasr_tie_context_phone(self._h, label.encode("latin-1"), state, C.byref(c)))
        return c.value

    def num_classes(self) -> int:
        return int(lib().aasr_tie_num_classes(self._h))

    def set_stats(self, gamma, sum_x, sum_xx) -> None:
        """aasr_scatter_get's layout: gamma [C], sum_x [C x dim], sum_xx [C x dim (dim + 1) / 2]."""
        g, sx = np.ascontiguousarray(gamma, np.float64), np.ascontiguousarray(sum_x, np.float64)
        sxx = np.ascontiguousarray(sum_xx, np.float64)
        n = self.num_classes()
        if g.shape != (n,) or sx.shape != (n, self.D) or sxx.shape != (n, self.D * (self.D + 1) // 2):
            raise ValueError("statistics do not match %d classes of %d dimensions" % (n, self.D))
        check(lib().aasr_tie_set_stats(self._h, _ptr(g), _ptr(sx), _ptr(sxx)))

    def set_occupancy(self, gamma) -> None:
        """Diagnostic, host only: the frame counts alone."""
        g = np.ascontiguousarray(gamma, np.float64)
        if g.shape != (self.num_classes(),):
            raise ValueError("one occupancy per class")
        check(lib().aasr_debug_tie_set_occupancy(self._h, _ptr(g)))

    def evaluate(self, jobs, cands=(), want_sums: bool = True):
        """jobs: [(members, masks)] with masks a 0/1 array [rows x len(members)]; cands: [(parent row, child 1 row,
        child 2 row or -1)] over the jobs' rows numbered through.  -> (sums [rows x E] or None, gains)."""
        job_k, job_rows, idx, words = [], [], [], []
        for members, masks in jobs:
            members = np.asarray(members, np.int32).reshape(-1)
            masks = np.asarray(masks, np.uint8).reshape(-1, len(members)) if len(members) else \
                np.zeros((np.asarray(masks).shape[0], 0), np.uint8)
            k, wpr = len(members), (len(members) + 31) // 32
            w = np.zeros((masks.shape[0], wpr), np.uint32)
            for b in range(k):
                w[:, b >> 5] |= (masks[:, b].astype(np.uint32) & 1) << np.uint32(b & 31)
            job_k.append(k)
            job_rows.append(masks.shape[0])
            idx.append(members)
            words.append(w.reshape(-1))
        job_k, job_rows = np.asarray(job_k, np.int32), np.asarray(job_rows, np.int32)
        idx = np.ascontiguousarray(np.concatenate(idx) if idx else np.zeros(0), np.int32)
        words = np.ascontiguousarray(np.concatenate(words) if words else np.zeros(0), np.uint32)
        cd = np.ascontiguousarray(np.asarray(cands, np.int32).reshape(-1, 3))
        rows = int(job_rows.sum())
        sums = np.zeros((rows, self.E)) if want_sums else None
        gain = np.zeros(len(cd))
        check(lib().aasr_tie_evaluate(self._h, len(job_k), _ptr(job_k), _ptr(job_rows), _ptr(idx) if len(idx) else None,
                                      _ptr(words) if len(words) else None, _ptr(sums), len(cd),
                                      _ptr(cd) if len(cd) else None, _ptr(gain) if len(cd) else None))
        return sums, gain

    def split(self, count: int = 100, sgain: float = 0.0, context: int = 1, hops: int = 1, info: int = 0) -> None:
        check(lib().aasr_tie_split(self._h, count, float(sgain), context, hops, info))

    def split_given(self, gain_of, count: int = 100, sgain: float = 0.0, context: int = 1) -> None:
        """Diagnostic, host only: the split loop with gain_of(members, new_set) -> gain in place of the device."""
        def fn(_user, nm, mem, ns, st):
            return float(gain_of([mem[i] for i in range(nm)], [st[i] for i in range(ns)]))
        check(lib().aasr_debug_tie_split_given(self._h, count, float(sgain), context, TIE_GAIN_FN(fn), None))

    def merge(self, mloss: float, info: int = 0) -> None:
        check(lib().aasr_tie_merge(self._h, float(mloss), info))

    def clusters(self):
        """The clusters in final order: [{"phone", "state", "index", "occ", "members", "rules"}]; rules: a list of
        rule sets, each [(rule name, context index, answer)]."""
        t = _take_text(lambda o, n: lib().aasr_tie_clusters_text(self._h, o, n)).decode("latin-1")
        out = []
        for line in t.split("\n")[:-1]:
            ph, st, si, occ, mem, rules = line.split("\x1f")
            sets = [[(r.rsplit(":", 2)[0], int(r.rsplit(":", 2)[1]), r.rsplit(":", 2)[2] == "1") for r in s.split(",")]
                    for s in rules.split("|")] if rules else []
            out.append({"phone": ph, "state": int(st), "index": int(si), "occ": float(occ),
                        "members": [int(m) for m in mem.split(",")] if mem else [], "rules": sets})
        return out

    def basebind(self, context: int = 1) -> bytes:
        return _take_text(lambda o, n: lib().aasr_tie_basebind_text(self._h, context, o, n))

    def write_basebind(self, path: str, context: int = 1) -> None:
        check(lib().aasr_tie_write_basebind(self._h, path.encode(), context))

    def write_model(self, base: str, context: int = 1) -> None:
        check(lib().aasr_tie_write_model(self._h, base.encode(), context))

    def shape(self) -> dict:
        """Diagnostic: the last batch's work items per hop, its sides and candidates; the rounds of the last runs."""
        out = (C.c_int32 * 6)()
        lib().aasr_debug_tie_shape(self._h, out)
        return dict(zip(("items_hop1", "items_hop2", "sides", "candidates", "rounds_split", "rounds_merge"), map(int, out)))


def run_tie_recipe(cfg_text: str, recipe_path: str, rule: str, out: Optional[str] = None, basebind: Optional[str] = None,
                   speakers: Optional[str] = None, opts: Optional[TieOptions] = None) -> dict:
    """The tie tool's run -> its counts and times."""
    opts = opts or TieOptions.defaults()
    opts.rule, opts.out = rule.encode(), (out.encode() if out else None)
    opts.basebind, opts.speakers = (basebind.encode() if basebind else None), (speakers.encode() if speakers else None)
    st = RunStats()
    check(lib().aasr_run_tie_recipe(cfg_text.encode(), recipe_path.encode(), C.byref(opts), C.byref(st)))
    return {"utterances": st.utterances, "frames": st.frames, "clusters": opts.clusters, "seconds_total": st.seconds_total,
            "seconds_features": opts.seconds_features, "seconds_scatter": opts.seconds_scatter,
            "seconds_split": opts.seconds_split, "seconds_merge": opts.seconds_merge}


# ---- state duration models (dur_est) -----------------------------------------------------------

class DurEstOptions(C.Structure):
    """aasr_dur_est_options"""
    _fields_ = [("ophn", C.c_int32), ("maxdur", C.c_int32), ("skip", C.c_int32), ("mincount", C.c_int32),
                ("info", C.c_int32), ("hist", C.c_char_p), ("gamma", C.c_char_p)]

    @classmethod
    def defaults(cls, **kw) -> "DurEstOptions":
        o = cls()
        lib().aasr_dur_est_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def run_dur_est(ph_path: str, recipe_path: str, hist: Optional[str] = None, gamma: Optional[str] = None,
                opts: Optional[DurEstOptions] = None) -> None:
    """The dur_est tool's run: duration histograms (hist) and their gamma fits (gamma, the .dur file).  Host only."""
    opts = opts or DurEstOptions.defaults()
    opts.hist, opts.gamma = (hist.encode() if hist else None), (gamma.encode() if gamma else None)
    check(lib().aasr_run_dur_est(ph_path.encode(), recipe_path.encode(), C.byref(opts)))


def dur_est_fit_gamma(hist) -> Optional[tuple]:
    """estimate_gamma_models on one histogram (hist[i]: occurrences of duration i + 1) -> (a, b), None with fewer than
    two points.  Host only."""
    h = np.ascontiguousarray(hist, np.int32)
    a, b = C.c_double(), C.c_double()
    return (a.value, b.value) if lib().aasr_dur_est_fit_gamma(_ptr(h), len(h), C.byref(a), C.byref(b)) else None


# ---- FST decoder (token passing over a search network) -------------------------------------------

AASR_FST_OK, AASR_FST_NO_TOKENS, AASR_FST_OVERFLOW_CANDIDATES, AASR_FST_OVERFLOW_RECOMB, AASR_FST_OVERFLOW_HISTORY = range(5)
FST_STATUS_NAMES = ("OK", "NO_TOKENS", "OVERFLOW_CANDIDATES", "OVERFLOW_RECOMB", "OVERFLOW_HISTORY")


class FstOptions(C.Structure):
    """aasr_fst_options"""
    _fields_ = [("beam", C.c_float), ("token_limit", C.c_int32), ("duration_scale", C.c_float),
                ("transition_scale", C.c_float), ("dur_by_state", C.c_int32), ("cap_candidates", C.c_int32),
                ("cap_recomb", C.c_int32), ("cap_history", C.c_int32)]

    @classmethod
    def defaults(cls, **kw) -> "FstOptions":
        o = cls()
        lib().aasr_fst_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


class FstNet:
    """aasr_fstnet: a "#FSTBasic MaxPlus" search network (Fst::read).  Host only."""

    def __init__(self, path: str):
        self._h = C.c_void_p()
        check(lib().aasr_fstnet_create_from_file(os.fsencode(path), C.byref(self._h)))
        L = lib()
        self.num_nodes, self.num_arcs = L.aasr_fstnet_num_nodes(self._h), L.aasr_fstnet_num_arcs(self._h)
        self.initial, self.max_pdf = L.aasr_fstnet_initial(self._h), L.aasr_fstnet_max_pdf(self._h)
        self.symbols = [L.aasr_fstnet_symbol(self._h, i) for i in range(L.aasr_fstnet_num_symbols(self._h))]

    @property
    def handle(self):
        return self._h

    def arrays(self) -> dict:
        a = {"arc_begin": np.zeros(self.num_nodes + 1, np.int32), "arc_tgt": np.zeros(self.num_arcs, np.int32),
             "arc_lp": np.zeros(self.num_arcs, np.float32), "arc_word": np.zeros(self.num_arcs, np.int32),
             "node_pdf": np.zeros(self.num_nodes, np.int32), "node_end": np.zeros(self.num_nodes, np.int32)}
        check(lib().aasr_fstnet_arrays(self._h, *[_ptr(a[k]) for k in ("arc_begin", "arc_tgt", "arc_lp", "arc_word", "node_pdf", "node_end")]))
        return a

    def close(self) -> None:
        if self._h:
            lib().aasr_fstnet_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FstDurations:
    """aasr_fst_durations: the .dur file of FstAcoustics::duration_read.  Host only."""

    def __init__(self, path: str):
        self._h = C.c_void_p()
        check(lib().aasr_fst_durations_read(os.fsencode(path), C.byref(self._h)))
        self.num_states = lib().aasr_fst_durations_num_states(self._h)

    @property
    def handle(self):
        return self._h

    def logprob(self, pdf: int, d: int, by_state: bool = False) -> np.float32:
        return np.float32(lib().aasr_fst_durations_logprob(self._h, 1 if by_state else 0, pdf, d))

    def close(self) -> None:
        if self._h:
            lib().aasr_fst_durations_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fst_batch_once(net: FstNet, dur, opts: FstOptions, n_frames, d_lna, lnabytes: int, n_models: int, row0, stream: int,
                    want_tokens: bool) -> list:
    L = lib()
    n = len(n_frames)
    T = np.ascontiguousarray(n_frames, np.int32)
    r0 = np.ascontiguousarray(row0, np.int64)
    n_rows = (d_lna.numel() * d_lna.element_size()) // (n_models * lnabytes)
    b = C.c_void_p()
    check(L.aasr_fst_batch_create(net.handle, dur.handle if dur is not None else None, C.byref(opts), n, _ptr(T), C.byref(b)))
    try:
        over = C.c_int32(0)
        check(L.aasr_fst_batch_dev(b, _ptr(d_lna), lnabytes, n_models, n_rows, _ptr(r0), stream))
        check(L.aasr_fst_batch_sync(b, stream, C.byref(over)))
        resolved = FstOptions()
        L.aasr_fst_batch_options(b, C.byref(resolved))
        out = []
        for u in range(n):
            st, nw, nt = C.c_int32(), C.c_int32(), C.c_int32()
            lp, blp, bflp = C.c_float(), C.c_float(), C.c_float()
            words = np.zeros(int(T[u]) + 1, np.int32)
            check(L.aasr_fst_batch_result(b, u, C.byref(st), C.byref(lp), C.byref(blp), C.byref(bflp), C.byref(nw), _ptr(words),
                                          len(words), C.byref(nt)))
            r = {"status": st.value, "logprob": np.float32(lp.value), "best_logprob": np.float32(blp.value),
                 "best_final_logprob": np.float32(bflp.value), "words": tuple(int(w) for w in words[:nw.value]),
                 "text": b" ".join(net.symbols[w] for w in words[:nw.value]), "n_tokens": nt.value,
                 "options": resolved, "device_bytes": L.aasr_fst_batch_device_bytes(b), "reran": False}
            if want_tokens:
                k = nt.value
                node, tl, td = np.zeros(k, np.int32), np.zeros(k, np.float32), np.zeros(k, np.int32)
                wb, tw = np.zeros(k + 1, np.int32), np.zeros(max(1, k * (int(T[u]) + 1)), np.int32)
                check(L.aasr_fst_batch_tokens(b, u, k, _ptr(node), _ptr(tl), _ptr(td), _ptr(wb), len(tw), _ptr(tw)))
                r["tokens"] = [(int(node[j]), np.float32(tl[j]), int(td[j]), tuple(int(w) for w in tw[wb[j]:wb[j + 1]]))
                               for j in range(k)]
            out.append(r)
        return out
    finally:
        L.aasr_fst_batch_destroy(b)


def fst_batch(net: FstNet, n_frames: list, d_lna, lnabytes: int, n_models: int, row0: list, opts: Optional[FstOptions] = None,
              dur: Optional[FstDurations] = None, stream: int = 0, want_tokens: bool = True, rerun: bool = True) -> list:
    """The FST token pass of a batch of utterances on the device.  d_lna: a device tensor (uint8, or float32 for
    lnabytes 4) of LNA rows, row0[u] the row of utterance u's first frame.  Per utterance a dict: status, logprob, words
    (ids), text (bytes), best_logprob, best_final_logprob, n_tokens and, with want_tokens, tokens: (node, logprob, dur,
    words) by descending log-probability.  With rerun the utterances that overflowed a capacity run once more in a batch of
    their own with every capacity doubled (`reran`); those that overflow again keep their overflow status."""
    opts = opts or FstOptions.defaults()
    out = _fst_batch_once(net, dur, opts, n_frames, d_lna, lnabytes, n_models, row0, stream, want_tokens)
    again = [u for u, r in enumerate(out) if r["status"] >= AASR_FST_OVERFLOW_CANDIDATES]
    if rerun and again:
        o2 = FstOptions()
        C.memmove(C.byref(o2), C.byref(out[again[0]]["options"]), C.sizeof(o2))
        o2.cap_candidates, o2.cap_recomb, o2.cap_history = 2 * o2.cap_candidates, 2 * o2.cap_recomb, 2 * o2.cap_history
        second = _fst_batch_once(net, dur, o2, [n_frames[u] for u in again], d_lna, lnabytes, n_models,
                                 [row0[u] for u in again], stream, want_tokens)
        for u, r in zip(again, second):
            r["reran"] = True
            out[u] = r
    return out


class FstStream:
    """aasr_fst_stream: n_sessions live searches over one network, fed frames as they arrive (include/aasr.h, "FST
    decoder: streaming sessions").  A session after t frames holds what fst_batch gives for an utterance of those t
    frames, whatever the feeds' sizes.  opts: FstOptions (None: the defaults); max_frames bounds every session's length
    and sizes its tables.  A status other than OK is sticky until reset(u); nothing is rerun."""

    def __init__(self, net: FstNet, n_sessions: int, max_frames: int, opts: Optional[FstOptions] = None,
                 dur: Optional[FstDurations] = None):
        self._h = C.c_void_p()
        self.net, self.dur = net, dur           # (both must outlive the handle)
        self.n_sessions, self.max_frames = n_sessions, max_frames
        opts = opts or FstOptions.defaults()
        check(lib().aasr_fst_stream_create(net.handle, dur.handle if dur is not None else None, C.byref(opts), n_sessions,
                                           max_frames, C.byref(self._h)))
        self.options = FstOptions()
        lib().aasr_fst_stream_options(self._h, C.byref(self.options))
        self.device_bytes = lib().aasr_fst_stream_device_bytes(self._h)

    def feed_dev(self, d_lna, lnabytes: int, n_models: int, row0: list, n_new: list, stream: int = 0) -> None:
        """queues one feed: session u takes n_new[u] frames from rows row0[u]... of the device tensor d_lna"""
        r0 = np.ascontiguousarray(row0, np.int64)
        nn = np.ascontiguousarray(n_new, np.int32)
        if len(r0) != self.n_sessions or len(nn) != self.n_sessions:
            raise ValueError("FstStream.feed_dev: row0 and n_new need one entry per session")
        n_rows = (d_lna.numel() * d_lna.element_size()) // (n_models * lnabytes) if n_models > 0 and lnabytes > 0 else 0
        check(lib().aasr_fst_stream_feed_dev(self._h, _ptr(d_lna), lnabytes, n_models, n_rows, _ptr(r0), _ptr(nn), stream))

    def sync(self, stream: int = 0) -> None:
        check(lib().aasr_fst_stream_sync(self._h, stream))

    def reset(self, u: int = -1) -> None:
        check(lib().aasr_fst_stream_reset(self._h, u))

    def result(self, u: int, want_tokens: bool = True) -> dict:
        """fst_batch's entry for the frames so far, plus partial_words, partial_text (the best token's words) and frames_done"""
        L = lib()
        st, fd, nw, npw, nt = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        lp, blp, bflp = C.c_float(), C.c_float(), C.c_float()
        words, part = np.zeros(self.max_frames + 1, np.int32), np.zeros(self.max_frames + 1, np.int32)
        check(L.aasr_fst_stream_result(self._h, u, C.byref(st), C.byref(fd), C.byref(lp), C.byref(blp), C.byref(bflp), C.byref(nw),
                                       _ptr(words), len(words), C.byref(npw), _ptr(part), len(part), C.byref(nt)))
        sym = self.net.symbols
        r = {"status": st.value, "logprob": np.float32(lp.value), "best_logprob": np.float32(blp.value),
             "best_final_logprob": np.float32(bflp.value), "words": tuple(int(w) for w in words[:nw.value]),
             "text": b" ".join(sym[w] for w in words[:nw.value]), "n_tokens": nt.value, "options": self.options,
             "device_bytes": self.device_bytes, "reran": False, "frames_done": fd.value,
             "partial_words": tuple(int(w) for w in part[:npw.value]),
             "partial_text": b" ".join(sym[w] for w in part[:npw.value])}
        if want_tokens:
            r["tokens"] = self.tokens(u, nt.value, fd.value)
        return r

    def tokens(self, u: int, n_tokens: Optional[int] = None, frames_done: Optional[int] = None) -> list:
        """(node, logprob, dur, words) of the session's tokens, by descending log-probability"""
        L = lib()
        if n_tokens is None or frames_done is None:
            nt, fd = C.c_int32(), C.c_int32()
            check(L.aasr_fst_stream_result(self._h, u, None, C.byref(fd), None, None, None, None, None, 0, None, None, 0, C.byref(nt)))
            n_tokens, frames_done = nt.value, fd.value
        k = n_tokens
        node, tl, td = np.zeros(max(1, k), np.int32), np.zeros(max(1, k), np.float32), np.zeros(max(1, k), np.int32)
        wb, tw = np.zeros(k + 2, np.int32), np.zeros(max(1, k * (frames_done + 1)), np.int32)
        check(L.aasr_fst_stream_tokens(self._h, u, k, _ptr(node), _ptr(tl), _ptr(td), _ptr(wb), len(tw), _ptr(tw)))
        return [(int(node[j]), np.float32(tl[j]), int(td[j]), tuple(int(w) for w in tw[wb[j]:wb[j + 1]])) for j in range(k)]

    def close(self) -> None:
        if self._h:
            lib().aasr_fst_stream_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FstDecodeOptions(C.Structure):
    """aasr_fst_decode_options"""
    _fields_ = [("fst", FstOptions), ("lna_files", C.c_int32), ("lnabytes", C.c_int32), ("group", C.c_int32),
                ("num_batches", C.c_int32), ("batch_index", C.c_int32), ("info", C.c_int32), ("speakers", C.c_void_p),
                ("out", C.c_char_p)]

    @classmethod
    def defaults(cls, **kw) -> "FstDecodeOptions":
        o = cls()
        lib().aasr_fst_decode_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def run_fst_decode_recipe(feat: Optional["Feat"], gmm: Optional["Gmm"], net: FstNet, recipe_path: str, out: str,
                          opts: Optional[FstDecodeOptions] = None, dur: Optional[FstDurations] = None,
                          speakers: Optional["SpeakerConfig"] = None) -> dict:
    """The fst_decode tool's run (aasr_run_fst_decode_recipe): engine mode from the recipe's audio= with feat and gmm, or
    opts.lna_files on its lna= files.  One line per utterance into `out`.  -> utterances, frames, seconds."""
    opts = opts or FstDecodeOptions.defaults()
    opts.out = os.fsencode(out)
    opts.speakers = speakers._h if speakers is not None else None
    st = RunStats()
    check(lib().aasr_run_fst_decode_recipe(feat._h if feat is not None else None, gmm._h if gmm is not None else None, net.handle,
                                           dur.handle if dur is not None else None, os.fsencode(recipe_path), C.byref(opts), C.byref(st)))
    return {"utterances": st.utterances, "frames": st.frames, "seconds_total": st.seconds_total, "seconds_device": st.seconds_device}


# ---- FST decoder: confidence (FstConfidence, FstConfidenceWithPhoneLoop) --------------------------

class FstConfOptions(C.Structure):
    """aasr_fst_conf_options"""
    _fields_ = [("grammar", FstOptions), ("phone", FstOptions), ("phone_loop", C.c_int32), ("verbose", C.c_int32)]

    @classmethod
    def defaults(cls, **kw) -> "FstConfOptions":
        o = cls()
        lib().aasr_fst_conf_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


class FstConfResult(C.Structure):
    """aasr_fst_conf_result"""
    _fields_ = [(k, C.c_float) for k in ("confidence", "token_conf", "ploop_conf", "edit_conf", "best_acu_conf", "grammar_logprob",
                                         "ploop_logprob", "best_final_logprob", "best_different_logprob", "best_acu_score")] + \
               [(k, C.c_int32) for k in ("frames", "grammar_status", "phone_status", "no_final", "valid")]


FST_CONF_FLOATS = tuple(k for k, t in FstConfResult._fields_ if t is C.c_float)


def fst_conf_remove_junk(s: bytes) -> bytes:
    """remove_junk of FstConfidence.cc: spaces and repeated consecutive bytes removed (the host's code)"""
    out = C.create_string_buffer(max(1, len(s)))
    n = lib().aasr_fst_conf_remove_junk(s, len(s), out, len(s))
    if n < 0:
        raise ValueError("aasr_fst_conf_remove_junk")
    return out.raw[:n]


def fst_conf_edit_distance(a: bytes, b: bytes) -> int:
    return lib().aasr_fst_conf_edit_distance(a, len(a), b, len(b))


def fst_conf_formulas(inputs: dict, n_words: int, grammar: bytes, ploop: Optional[bytes]) -> dict:
    """The host's formulas on given raw inputs (grammar_logprob, ploop_logprob, best_final_logprob, best_different_logprob,
    best_acu_score, frames); ploop None: the plain FstConfidence."""
    r = FstConfResult()
    for k, v in inputs.items():
        setattr(r, k, v)
    lib().aasr_fst_conf_formulas(C.byref(r), n_words, grammar, len(grammar), ploop, len(ploop) if ploop is not None else 0)
    return {k: np.float32(getattr(r, k)) for k in FST_CONF_FLOATS}


def _fst_inner_result(L, b, net: FstNet, u: int, T: int, want_tokens: bool) -> dict:
    st, nw, nt = C.c_int32(), C.c_int32(), C.c_int32()
    lp, blp, bflp = C.c_float(), C.c_float(), C.c_float()
    words = np.zeros(T + 1, np.int32)
    check(L.aasr_fst_batch_result(b, u, C.byref(st), C.byref(lp), C.byref(blp), C.byref(bflp), C.byref(nw), _ptr(words), len(words), C.byref(nt)))
    r = {"status": st.value, "logprob": np.float32(lp.value), "best_logprob": np.float32(blp.value),
         "best_final_logprob": np.float32(bflp.value), "words": tuple(int(w) for w in words[:nw.value]),
         "text": b" ".join(net.symbols[w] for w in words[:nw.value]), "n_tokens": nt.value}
    if want_tokens:
        k = nt.value
        node, tl, td = np.zeros(k, np.int32), np.zeros(k, np.float32), np.zeros(k, np.int32)
        wb, tw = np.zeros(k + 1, np.int32), np.zeros(max(1, k * (T + 1)), np.int32)
        check(L.aasr_fst_batch_tokens(b, u, k, _ptr(node), _ptr(tl), _ptr(td), _ptr(wb), len(tw), _ptr(tw)))
        r["tokens"] = [(int(node[j]), np.float32(tl[j]), int(td[j]), tuple(int(w) for w in tw[wb[j]:wb[j + 1]])) for j in range(k)]
    return r


def _fst_conf_batch_once(net, phone_net, dur, opts, n_frames, d_lna, lnabytes, n_models, row0, stream, want_tokens) -> list:
    L = lib()
    n = len(n_frames)
    T = np.ascontiguousarray(n_frames, np.int32)
    r0 = np.ascontiguousarray(row0, np.int64)
    n_rows = (d_lna.numel() * d_lna.element_size()) // (n_models * lnabytes)
    b = C.c_void_p()
    check(L.aasr_fst_conf_batch_create(net.handle, phone_net.handle if phone_net is not None else None,
                                       dur.handle if dur is not None else None, C.byref(opts), n, _ptr(T), C.byref(b)))
    try:
        over = C.c_int32(0)
        check(L.aasr_fst_conf_batch_dev(b, _ptr(d_lna), lnabytes, n_models, n_rows, _ptr(r0), stream))
        check(L.aasr_fst_conf_batch_sync(b, stream, C.byref(over)))
        resolved = FstConfOptions()
        L.aasr_fst_conf_batch_options(b, C.byref(resolved))
        inner = [(L.aasr_fst_conf_batch_grammar(b), net, "grammar"), (L.aasr_fst_conf_batch_phone(b), phone_net, "phone")]
        out = []
        for u in range(n):
            cr = FstConfResult()
            check(L.aasr_fst_conf_batch_result(b, u, C.byref(cr)))
            r = {k: np.float32(getattr(cr, k)) for k in FST_CONF_FLOATS}
            r.update(frames=cr.frames, grammar_status=cr.grammar_status, phone_status=cr.phone_status, no_final=cr.no_final,
                     valid=cr.valid, options=resolved, reran=False)
            if not cr.valid:
                r["confidence"] = None
            for k, (h, nt, name) in enumerate(inner):
                if not h:
                    r[name] = None
                    continue
                r[name] = _fst_inner_result(L, h, nt, u, int(T[u]), want_tokens)
                hf, nw, hd = C.c_int32(), C.c_int32(), C.c_int32()
                bf, bd = C.c_float(), C.c_float()
                check(L.aasr_fst_conf_batch_record(b, u, k, C.byref(hf), C.byref(nw), C.byref(hd), C.byref(bf), C.byref(bd)))
                r[name]["record"] = {"has_final": hf.value, "n_words": nw.value, "has_different": hd.value,
                                     "best_final_logprob": np.float32(bf.value), "best_different_logprob": np.float32(bd.value)}
            r["text"] = r["grammar"]["text"]
            out.append(r)
        return out
    finally:
        L.aasr_fst_conf_batch_destroy(b)


def fst_conf_batch(net: FstNet, phone_net: Optional[FstNet], n_frames: list, d_lna, lnabytes: int, n_models: int, row0: list,
                   opts: Optional[FstConfOptions] = None, dur: Optional[FstDurations] = None, stream: int = 0,
                   want_tokens: bool = False, rerun: bool = True) -> list:
    """The confidence of a batch of utterances on the device (aasr_fst_conf_batch_*): the grammar search, with
    opts.phone_loop the search over phone_net on the same acoustics, the frame-best sums and the token records.  Per
    utterance a dict: the ten floats of aasr_fst_conf_result (confidence None when a search overflowed), frames,
    grammar_status, phone_status, no_final, valid, text, and `grammar` / `phone` (None without a phone loop): the search's
    result as fst_batch gives it plus `record`, the device's token record.  With rerun the utterances that overflowed a
    capacity run once more with every capacity of both searches doubled (`reran`)."""
    opts = opts or FstConfOptions.defaults()
    out = _fst_conf_batch_once(net, phone_net, dur, opts, n_frames, d_lna, lnabytes, n_models, row0, stream, want_tokens)
    again = [u for u, r in enumerate(out) if not r["valid"]]
    if rerun and again:
        o2 = FstConfOptions()
        C.memmove(C.byref(o2), C.byref(out[again[0]]["options"]), C.sizeof(o2))
        for o in (o2.grammar, o2.phone):
            o.cap_candidates, o.cap_recomb, o.cap_history = 2 * o.cap_candidates, 2 * o.cap_recomb, 2 * o.cap_history
        second = _fst_conf_batch_once(net, phone_net, dur, o2, [n_frames[u] for u in again], d_lna, lnabytes, n_models,
                                      [row0[u] for u in again], stream, want_tokens)
        for u, r in zip(again, second):
            r["reran"] = True
            out[u] = r
    return out


def fst_frame_best(n_frames: list, d_lna, lnabytes: int, n_models: int, row0: list, net: FstNet, stream: int = 0):
    """The frame-best pass alone (aasr_fst_conf_batch_frame_best_dev): per utterance (float32 [frames] of the frames' best
    acoustic values, their float32 sum in frame order).  net: any network (the batch is made over it and not searched)."""
    L = lib()
    n = len(n_frames)
    T = np.ascontiguousarray(n_frames, np.int32)
    r0 = np.ascontiguousarray(row0, np.int64)
    n_rows = (d_lna.numel() * d_lna.element_size()) // (n_models * lnabytes)
    b = C.c_void_p()
    opts = FstConfOptions.defaults()
    check(L.aasr_fst_conf_batch_create(net.handle, None, None, C.byref(opts), n, _ptr(T), C.byref(b)))
    try:
        check(L.aasr_fst_conf_batch_frame_best_dev(b, _ptr(d_lna), lnabytes, n_models, n_rows, _ptr(r0), stream))
        out = []
        for u in range(n):
            best, s = np.zeros(int(T[u]), np.float32), C.c_float()
            check(L.aasr_fst_conf_batch_frame_best(b, u, stream, _ptr(best), len(best), C.byref(s)))
            out.append((best, np.float32(s.value)))
        return out
    finally:
        L.aasr_fst_conf_batch_destroy(b)


class FstConfStream:
    """aasr_fst_conf_stream: n_sessions live confidences, fed frames as they arrive (include/aasr.h, "FST decoder:
    confidence on streaming sessions").  A session after t frames answers what fst_conf_batch gives for an utterance of
    those t frames, whatever the feeds' sizes.  opts: FstConfOptions (None: the defaults; phone_loop is set from
    phone_net); max_frames bounds every session's length and sizes both searches' tables.  A search's status other than
    OK is sticky until reset(u); nothing is rerun."""

    def __init__(self, net: FstNet, phone_net: Optional[FstNet], n_sessions: int, max_frames: int,
                 opts: Optional[FstConfOptions] = None, dur: Optional[FstDurations] = None):
        self._h = C.c_void_p()
        self.net, self.phone_net, self.dur = net, phone_net, dur           # (all must outlive the handle)
        self.n_sessions, self.max_frames = n_sessions, max_frames
        opts = opts or FstConfOptions.defaults(phone_loop=1 if phone_net is not None else 0)
        check(lib().aasr_fst_conf_stream_create(net.handle, phone_net.handle if phone_net is not None else None,
                                                dur.handle if dur is not None else None, C.byref(opts), n_sessions, max_frames,
                                                C.byref(self._h)))
        self.options = FstConfOptions()
        lib().aasr_fst_conf_stream_options(self._h, C.byref(self.options))
        self.device_bytes = lib().aasr_fst_conf_stream_device_bytes(self._h)
        self._nets = (net, phone_net if self.options.phone_loop else None)

    def feed_dev(self, d_lna, lnabytes: int, n_models: int, row0: list, n_new: list, stream: int = 0) -> None:
        """queues one feed: session u takes n_new[u] frames from rows row0[u]... of the device tensor d_lna"""
        r0 = np.ascontiguousarray(row0, np.int64)
        nn = np.ascontiguousarray(n_new, np.int32)
        if len(r0) != self.n_sessions or len(nn) != self.n_sessions:
            raise ValueError("FstConfStream.feed_dev: row0 and n_new need one entry per session")
        n_rows = (d_lna.numel() * d_lna.element_size()) // (n_models * lnabytes) if n_models > 0 and lnabytes > 0 else 0
        check(lib().aasr_fst_conf_stream_feed_dev(self._h, _ptr(d_lna), lnabytes, n_models, n_rows, _ptr(r0), _ptr(nn), stream))

    def sync(self, stream: int = 0) -> None:
        check(lib().aasr_fst_conf_stream_sync(self._h, stream))

    def reset(self, u: int = -1) -> None:
        check(lib().aasr_fst_conf_stream_reset(self._h, u))

    def search_result(self, u: int, phone: int = 0, want_tokens: bool = False) -> dict:
        """FstStream.result's entry for the grammar search (phone 0) or the phone-loop search (phone 1), plus `record`"""
        L = lib()
        st, fd, nw, npw, nt = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        lp, blp, bflp = C.c_float(), C.c_float(), C.c_float()
        words, part = np.zeros(self.max_frames + 1, np.int32), np.zeros(self.max_frames + 1, np.int32)
        check(L.aasr_fst_conf_stream_search_result(self._h, u, phone, C.byref(st), C.byref(fd), C.byref(lp), C.byref(blp), C.byref(bflp),
                                                   C.byref(nw), _ptr(words), len(words), C.byref(npw), _ptr(part), len(part), C.byref(nt)))
        sym = self._nets[phone].symbols
        r = {"status": st.value, "logprob": np.float32(lp.value), "best_logprob": np.float32(blp.value),
             "best_final_logprob": np.float32(bflp.value), "words": tuple(int(w) for w in words[:nw.value]),
             "text": b" ".join(sym[w] for w in words[:nw.value]), "n_tokens": nt.value, "frames_done": fd.value,
             "partial_words": tuple(int(w) for w in part[:npw.value]),
             "partial_text": b" ".join(sym[w] for w in part[:npw.value])}
        hf, rw, hd = C.c_int32(), C.c_int32(), C.c_int32()
        bf, bd = C.c_float(), C.c_float()
        check(L.aasr_fst_conf_stream_record(self._h, u, phone, C.byref(hf), C.byref(rw), C.byref(hd), C.byref(bf), C.byref(bd)))
        r["record"] = {"has_final": hf.value, "n_words": rw.value, "has_different": hd.value,
                       "best_final_logprob": np.float32(bf.value), "best_different_logprob": np.float32(bd.value)}
        if want_tokens:
            r["tokens"] = self.tokens(u, phone, nt.value, fd.value)
        return r

    def tokens(self, u: int, phone: int = 0, n_tokens: Optional[int] = None, frames_done: Optional[int] = None) -> list:
        """(node, logprob, dur, words) of a search's tokens, by descending log-probability"""
        L = lib()
        if n_tokens is None or frames_done is None:
            nt, fd = C.c_int32(), C.c_int32()
            check(L.aasr_fst_conf_stream_search_result(self._h, u, phone, None, C.byref(fd), None, None, None, None, None, 0, None, None, 0,
                                                       C.byref(nt)))
            n_tokens, frames_done = nt.value, fd.value
        k = n_tokens
        node, tl, td = np.zeros(max(1, k), np.int32), np.zeros(max(1, k), np.float32), np.zeros(max(1, k), np.int32)
        wb, tw = np.zeros(k + 2, np.int32), np.zeros(max(1, k * (frames_done + 1)), np.int32)
        check(L.aasr_fst_conf_stream_tokens(self._h, u, phone, k, _ptr(node), _ptr(tl), _ptr(td), _ptr(wb), len(tw), _ptr(tw)))
        return [(int(node[j]), np.float32(tl[j]), int(td[j]), tuple(int(w) for w in tw[wb[j]:wb[j + 1]])) for j in range(k)]

    def best_acu(self, u: int):
        """(the carried float32 sum of the frames' best acoustic values, the frames it covers); with a phone loop only"""
        s, n = C.c_float(), C.c_int32()
        check(lib().aasr_fst_conf_stream_best_acu(self._h, u, C.byref(s), C.byref(n)))
        return np.float32(s.value), n.value

    def result(self, u: int, want_tokens: bool = False) -> dict:
        """fst_conf_batch's entry for the frames fed so far (without `reran`: nothing is rerun on a stream)"""
        cr = FstConfResult()
        check(lib().aasr_fst_conf_stream_result(self._h, u, C.byref(cr)))
        r = {k: np.float32(getattr(cr, k)) for k in FST_CONF_FLOATS}
        r.update(frames=cr.frames, grammar_status=cr.grammar_status, phone_status=cr.phone_status, no_final=cr.no_final,
                 valid=cr.valid, options=self.options, reran=False)
        if not cr.valid:
            r["confidence"] = None
        r["grammar"] = self.search_result(u, 0, want_tokens)
        r["phone"] = self.search_result(u, 1, want_tokens) if self._nets[1] is not None else None
        r["text"] = r["grammar"]["text"]
        return r

    def close(self) -> None:
        if self._h:
            lib().aasr_fst_conf_stream_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FstConfidenceOptions(C.Structure):
    """aasr_fst_confidence_options"""
    _fields_ = [("decode", FstDecodeOptions), ("phone", FstOptions), ("phone_loop", C.c_int32)]

    @classmethod
    def defaults(cls, **kw) -> "FstConfidenceOptions":
        o = cls()
        lib().aasr_fst_confidence_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o


def run_fst_confidence_recipe(feat: Optional["Feat"], gmm: Optional["Gmm"], net: FstNet, phone_net: Optional[FstNet], recipe_path: str,
                              out: str, opts: Optional[FstConfidenceOptions] = None, dur: Optional[FstDurations] = None,
                              speakers: Optional["SpeakerConfig"] = None) -> dict:
    """fst_decode --confidence (aasr_run_fst_confidence_recipe): as run_fst_decode_recipe, a confidence behind every
    log-probability; opts.phone_loop is set from phone_net."""
    opts = opts or FstConfidenceOptions.defaults()
    opts.decode.out = os.fsencode(out)
    opts.decode.speakers = speakers._h if speakers is not None else None
    opts.phone_loop = 1 if phone_net is not None else 0
    st = RunStats()
    check(lib().aasr_run_fst_confidence_recipe(feat._h if feat is not None else None, gmm._h if gmm is not None else None, net.handle,
                                               phone_net.handle if phone_net is not None else None,
                                               dur.handle if dur is not None else None, os.fsencode(recipe_path), C.byref(opts), C.byref(st)))
    return {"utterances": st.utterances, "frames": st.frames, "seconds_total": st.seconds_total, "seconds_device": st.seconds_device}
