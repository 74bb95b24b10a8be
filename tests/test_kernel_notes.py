"""The scoring kernels' register budget, read from the code object's notes (no GPU needed).

k_gmm_diag_score_pl sits at the register wall of the two-waves-per-SIMD form: the frame operand (80 VGPRs), two
accumulator sets (64), two fragment sets.  Round 3's bench instance had grown to 256 VGPRs + 24 spilled ones (all in
its prologue); since the frame operand is formed by k_frame_operand and only loaded here, the instances have no scratch
at all -- and a spill that enters the tile loop would cost far more than the few percent any scheduling change gains,
silently.  So the build fails this test when the bench instance (or any two-term instance the default paths launch)
starts to use scratch memory."""
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _scoring_objects():
    """the objects of the scoring unit's files: one per csrc/gmm_score*.hip (the map of the files: gmm_score.hip)"""
    srcs = sorted(glob.glob(os.path.join(ROOT, "aaltoasr_amd", "csrc", "gmm_score*.hip")))
    assert os.path.join(ROOT, "aaltoasr_amd", "csrc", "gmm_score.hip") in srcs and len(srcs) > 1, srcs
    objs = [os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", os.path.basename(s) + ".o") for s in srcs]
    for obj in objs:
        assert os.path.exists(obj), obj
    return objs


@pytest.fixture(scope="module")
def notes(capi):
    import kernel_notes
    out = {}
    for obj in _scoring_objects():
        out.update(kernel_notes.kernel_notes(obj))
    return out


def test_no_scoring_kernel_is_instantiated_in_two_files(capi):
    """Every kernel instance of the scoring unit lives in exactly one of its files: a second copy would be compiled,
    shipped and loaded twice, and the `notes` dictionary above would hide one of them."""
    import kernel_notes
    seen = {}
    for obj in _scoring_objects():
        for name in kernel_notes.kernel_notes(obj):
            seen.setdefault(name, []).append(os.path.basename(obj))
    twice = {n: o for n, o in seen.items() if len(o) > 1}
    assert not twice, twice


def _get(notes, name):
    hits = [v for k, v in notes.items() if k.endswith(name)]
    assert len(hits) == 1, (name, len(hits))
    return hits[0]


def test_bench_instance_has_no_scratch(notes):
    # configs[1] / configs[2]: 39 dimensions (NK16 = 5), grouped tracks, unmasked, 8-wave form, two fp16 terms
    k = _get(notes, "k_gmm_diag_score_pl<5, true, false, true, 2, false, false>")
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0, k
    assert k["vgpr"] <= 232 and k["agpr"] == 0, k          # 206 when this was written; 256 is the wall


@pytest.mark.parametrize("inst", [
    "k_gmm_diag_score_pl<5, true, true, true, 2, false, false>",    # the clustered (masked) pass
    "k_gmm_diag_score_pl<5, true, false, false, 2, false, false>",  # small batches: 4-wave form
    "k_gmm_diag_score_pl<5, true, false, true, 2, true, false>",    # engine parts: pivot groups, operand formed in the prologue
    "k_gmm_diag_score_pl<5, true, true, true, 2, true, false>",     # ... under Gaussian clustering
    "k_gmm_diag_score_pl<6, true, false, true, 2, true, false>",    # ... the slab-constant part (six slabs at 39 dimensions)
    "k_gmm_diag_score_pl<5, true, false, true, 2, false, true>",    # outlier routing merged in the close logic
    "k_gmm_diag_score_pl<5, false, false, true, 2, false, false>",  # independent tracks
])
def test_two_term_instances_of_the_default_paths_have_no_scratch(notes, inst):
    k = _get(notes, inst)
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0, (inst, k)


def test_every_dimension_instance_of_the_bench_form_has_no_scratch(notes):
    bad = {n: k for n, k in notes.items()
           if "k_gmm_diag_score_pl<" in n and (n.endswith(", 2, false, false>") or n.endswith(", 2, true, false>")) and
           (k["scratch"] or k["spill_vgpr"])}
    assert not bad, bad


def test_feature_kernels_keep_four_waves_per_simd():
    """k_spectral_fused is bound by vector issue with four workgroups per CU (four waves per SIMD): 128 VGPRs is the
    wall (round 4 measured a variant at 133: one workgroup fewer per CU), and nothing of the three production kernels
    may sit in scratch memory."""
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "feat_kernels.hip.o")
    assert os.path.exists(obj)
    notes = kernel_notes.kernel_notes(obj)
    spectral = [v for k, v in notes.items() if k.endswith("k_spectral_fused")]
    assert len(spectral) == 1 and spectral[0]["vgpr"] <= 128 and spectral[0]["scratch"] == 0, spectral
    for name in ("k_temporal_fused<64, 512>", "k_mean_subtract_tiled<128, float, 512>", "k_mean_subtract_tiled<64, float, 256>"):
        hits = [v for k, v in notes.items() if k.endswith(name)]
        assert len(hits) == 1 and hits[0]["scratch"] == 0 and hits[0]["spill_vgpr"] == 0 and hits[0]["vgpr"] <= 128, (name, hits)


# ---- the statistics accumulation kernel (csrc/stats_accum.hip) ----------------------------------------------------
# k_stats_items<DIMP> holds a frame as DIMP doubles per lane (2 DIMP VGPRs) next to its running sums; one instance per
# padded dimension of gmm_build_f64.

STATS_DIMS = (8, 16, 24, 32, 40, 48, 64, 96, 128, 192)


@pytest.fixture(scope="module")
def stats_notes(capi):
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "stats_accum.hip.o")
    assert os.path.exists(obj)
    notes = kernel_notes.kernel_notes(obj)
    return {n: _get(notes, "k_stats_items<%d>" % n) for n in STATS_DIMS}


def test_stats_instances_up_to_128_have_no_scratch(stats_notes):
    for n in STATS_DIMS[:-1]:
        k = stats_notes[n]
        assert k["scratch"] == 0 and k["spill_vgpr"] == 0, (n, k)
        assert k["vgpr"] <= 512, (n, k)     # the unified file of a 256-thread workgroup (338 at <128> when written)


def test_stats_instances_of_real_front_ends_stay_in_plain_vgprs(stats_notes):
    """24 ... 48 padded dimensions (the 39-dimensional front end runs <40>): no scratch, no spilled VGPR, no AGPR
    copies, and at most 168 VGPRs -- three waves per SIMD (111 / 127 / 143 / 160 when this was written)."""
    for n in (24, 32, 40, 48):
        k = stats_notes[n]
        assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["agpr"] == 0 and k["vgpr"] <= 168, (n, k)


def test_stats_192_spill_does_not_grow(stats_notes):
    """<192> is the one instance that spills: its frame alone is 384 VGPRs, the notes say 512 registers (256 + 256
    AGPRs), 97 spilled VGPRs and 248 bytes of scratch per lane ("ML statistics").  It is correct as it is
    (tests/test_stats_shapes_gpu.py runs it); this keeps the spill from growing unnoticed.  Less is welcome."""
    k = stats_notes[192]
    assert k["scratch"] <= 248 and k["spill_vgpr"] <= 97, k
