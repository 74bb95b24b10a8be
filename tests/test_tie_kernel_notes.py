"""The state-tying kernels' budgets, read from the code object's notes (no GPU needed).

k_tie_masked_sum keeps TIE_NE = 4 result tiles of the FP64 matrix pipe in registers over a job's whole member list and
reads both operands from global memory; k_tie_logdet<MD> keeps one covariance of up to MD dimensions in LDS -- declared
in the kernel, the launch asks for no dynamic LDS on top -- and walks it with a lane per row, so nothing of either may
live in scratch memory: a spilled tile or a matrix row indexed through scratch would be read and written around every
step of the factorization.  63 dimensions must stay within 32 KiB, so that five waves share a CU's LDS."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (VGPRs, AGPRs) of the build this was written with: upper bounds
LOGDET = {16: (64, 0), 32: (64, 0), 48: (64, 0), 63: (64, 0)}
SMALL = {"k_tie_masked_sum": (96, 32), "k_tie_pack": (8, 0), "k_tie_gain": (24, 0)}


@pytest.fixture(scope="module")
def notes(capi):
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "tie_split.hip.o")
    assert os.path.exists(obj)
    return kernel_notes.kernel_notes(obj)


def _one(notes, name):
    hits = [v for k, v in notes.items() if k.split("::")[-1] == name]
    assert len(hits) == 1, (name, sorted(notes))
    return hits[0]


def test_every_tie_kernel_is_covered(notes):
    names = sorted(k.split("::")[-1] for k in notes if "k_tie" in k)
    assert names == sorted(["k_tie_logdet<%d>" % md for md in LOGDET] + list(SMALL)), names


@pytest.mark.parametrize("md", sorted(LOGDET))
def test_factorization_instances_have_no_scratch_and_stay_within_their_lds(notes, md):
    k = _one(notes, "k_tie_logdet<%d>" % md)
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0, k
    vgpr, agpr = LOGDET[md]
    assert k["vgpr"] <= vgpr and k["agpr"] <= agpr, k
    # the matrix (row stride md | 1) and the 64 means, nothing else but alignment; at most 32 KiB
    want = md * (md | 1) * 8 + 64 * 8
    assert want <= k["lds"] <= want + 64 and k["lds"] <= 32 * 1024, k


@pytest.mark.parametrize("name", sorted(SMALL))
def test_sum_pack_and_gain_kernels(notes, name):
    k = _one(notes, name)
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0 and k["lds"] == 0, k
    vgpr, agpr = SMALL[name]
    assert k["vgpr"] <= vgpr and k["agpr"] <= agpr, k
    assert k["vgpr"] + k["agpr"] <= 128, k      # four waves a SIMD
