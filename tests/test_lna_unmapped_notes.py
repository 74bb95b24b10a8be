"""The condition the chunked score + LNA step (csrc/gmm_score_lna.cc) rests on, read from the code objects' notes (no GPU
needed): an LNA workgroup of the unmapped instance fits on a CU BESIDE a scoring workgroup of the bench form.

Per SIMD the scoring workgroup (8 waves, two per SIMD) holds 2 x its VGPR count rounded up to the allocation granule of 8;
an LNA workgroup (4 waves, one per SIMD) needs its own count out of the 512.  With the column map in registers the <13>
instance took 112 VGPRs against the 96 that are left: its waves were only ever placed in the gaps between scoring rounds,
and two streams ran one after the other.  A later edit that pushes either kernel over the line would do the same,
silently -- so it fails here."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

VGPR_FILE = 512          # per SIMD lane, gfx950
VGPR_GRANULE = 8
LDS_PER_CU = 160 * 1024
LNA_LDS = 64             # __shared__ double red[8]
BENCH_SCORING = "k_gmm_diag_score_pl<5, true, false, true, 2, false, false>"


def _one(notes, name):
    hits = [v for k, v in notes.items() if k.endswith(name)]
    assert len(hits) == 1, (name, sorted(notes))
    return hits[0]


@pytest.fixture(scope="module")
def lna_notes(capi):
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "lna_encode.hip.o")
    assert os.path.exists(obj), obj
    return kernel_notes.kernel_notes(obj)


@pytest.fixture(scope="module")
def scoring(capi):
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "gmm_score_f16x2.hip.o")
    assert os.path.exists(obj), obj
    return _one(kernel_notes.kernel_notes(obj), BENCH_SCORING)


def test_unmapped_13_fits_the_registers_scoring_leaves(lna_notes):
    k = _one(lna_notes, "k_state_norm_lna_reg<13, false>")
    assert k["vgpr"] <= 96 and k["agpr"] == 0, k          # 90 when this was written (the mapped instance: 112)
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0, k
    assert k["lds"] == LNA_LDS, k


@pytest.mark.parametrize("vpt", [4, 8, 10, 13, 16])
def test_both_forms_of_every_instance_exist_without_scratch(lna_notes, vpt):
    for mapped in ("true", "false"):
        k = _one(lna_notes, "k_state_norm_lna_reg<%d, %s>" % (vpt, mapped))
        assert k["scratch"] == 0 and k["spill_vgpr"] == 0, (vpt, mapped, k)
    # the unmapped form never needs more registers than the mapped one
    assert _one(lna_notes, "k_state_norm_lna_reg<%d, false>" % vpt)["vgpr"] <= \
        _one(lna_notes, "k_state_norm_lna_reg<%d, true>" % vpt)["vgpr"]


def test_lna_workgroup_fits_beside_the_bench_scoring_workgroup(capi, lna_notes, scoring):
    lna = _one(lna_notes, "k_state_norm_lna_reg<13, false>")
    up = lambda n: (n + VGPR_GRANULE - 1) // VGPR_GRANULE * VGPR_GRANULE
    assert scoring["agpr"] == 0, scoring
    assert 2 * up(scoring["vgpr"]) + up(lna["vgpr"]) <= VGPR_FILE, (scoring, lna)
    fn = capi.lib().aasr_debug_pl_bench_smem_bytes
    fn.argtypes = [__import__("ctypes").c_int]
    smem = fn(1)                                            # dynamic LDS of the 8-wave form; the notes hold the static part
    assert smem > 0
    assert smem + scoring["lds"] + LNA_LDS <= LDS_PER_CU, (smem, scoring)
