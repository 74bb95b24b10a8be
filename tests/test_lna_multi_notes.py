"""The budget of the multi-frame LNA kernel (csrc/lna_encode.hip: k_state_norm_lna_multi<VPT, Q>), read from the code
objects' notes (no GPU needed).  The chunked score + LNA step (csrc/gmm_score_lna.cc) runs its LNA segments BESIDE a
scoring workgroup of the bench form, so every instance the dispatcher can pick there has to fit into what that workgroup
leaves on a CU:

  - registers: the scoring workgroup holds two waves per SIMD, each its VGPR count rounded up to the granule of 8; an LNA
    wave needs its own count, rounded up, out of the 512;
  - no scratch and no spills, of vector or of scalar registers;
  - LDS: its own (the reduction slots and the parked row) plus the scoring kernel's static and dynamic LDS within 160 KB.

The one-frame instances the dispatcher falls back to (another S, a column map, a float output, 4-byte codes, Q = 1) still
exist."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

VGPR_FILE = 512
VGPR_GRANULE = 8
LDS_PER_CU = 160 * 1024
BENCH_SCORING = "k_gmm_diag_score_pl<5, true, false, true, 2, false, false>"
MULTI = [(13, 4), (13, 2)]            # every instance lna_encode_launch_grid can pick


def _one(notes, name):
    hits = [v for k, v in notes.items() if k.endswith(name)]
    assert len(hits) == 1, (name, sorted(notes))
    return hits[0]


def _up(n):
    return (n + VGPR_GRANULE - 1) // VGPR_GRANULE * VGPR_GRANULE


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


def test_the_dispatcher_has_no_other_multi_frame_instance(lna_notes):
    names = sorted(k for k in lna_notes if "k_state_norm_lna_multi" in k)
    assert len(names) == len(MULTI), names
    for vpt, q in MULTI:
        _one(lna_notes, "k_state_norm_lna_multi<%d, %d>" % (vpt, q))


@pytest.mark.parametrize("vpt,q", MULTI)
def test_instance_fits_beside_the_bench_scoring_workgroup(capi, lna_notes, scoring, vpt, q):
    k = _one(lna_notes, "k_state_norm_lna_multi<%d, %d>" % (vpt, q))
    assert scoring["agpr"] == 0 and k["agpr"] == 0, (scoring, k)
    assert 2 * _up(scoring["vgpr"]) + _up(k["vgpr"]) <= VGPR_FILE, (scoring, k)
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0, k
    fn = capi.lib().aasr_debug_pl_bench_smem_bytes
    fn.argtypes = [ctypes.c_int]
    smem = fn(1)                      # dynamic LDS of the 8-wave form; the notes hold the static part
    assert smem > 0
    assert k["lds"] > 0
    assert smem + scoring["lds"] + k["lds"] <= LDS_PER_CU, (smem, scoring, k)


@pytest.mark.parametrize("vpt", [4, 8, 10, 13, 16])
def test_one_frame_instances_still_exist(lna_notes, vpt):
    for mapped in ("true", "false"):
        k = _one(lna_notes, "k_state_norm_lna_reg<%d, %s>" % (vpt, mapped))
        assert k["scratch"] == 0 and k["spill_vgpr"] == 0, (vpt, mapped, k)
