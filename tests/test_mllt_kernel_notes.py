"""The MLLT kernels' register budget, read from the code object's notes (no GPU needed).

k_mllt_gsum<PB> keeps MLLT_NE x PB result tiles of the FP64 matrix pipe in registers for a whole item of 256 Gaussians
and reads both operands straight from global memory, no LDS: a tile that went to scratch memory would be read and
written around every matrix instruction.  k_mllt_var<PB> keeps sixteen variance sums a lane -- the rows of A a wave
owns -- whatever the dimension, and reads its coefficients at wave-uniform addresses; indexed by a runtime row they
would become an array in scratch.  So every instance must stay free of scratch and of spills."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (VGPRs, AGPRs, LDS bytes) of the build this was written with: upper bounds
GSUM = {1: (84, 16, 0), 2: (108, 32, 0), 3: (128, 48, 0), 4: (104, 64, 0)}
VAR = {1: (52, 0, 0), 2: (52, 0, 0), 3: (52, 0, 0), 4: (52, 0, 0)}
SMALL = {"k_mllt_cov": (18, 0, 0), "k_mllt_slab_add": (8, 0, 0)}


@pytest.fixture(scope="module")
def notes(capi):
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "mllt.hip.o")
    assert os.path.exists(obj)
    return kernel_notes.kernel_notes(obj)


def _one(notes, name):
    hits = [v for k, v in notes.items() if k.split("::")[-1] == name]
    assert len(hits) == 1, (name, sorted(notes))
    return hits[0]


def test_every_mllt_kernel_is_covered(notes):
    names = sorted(k.split("::")[-1] for k in notes if "k_mllt" in k)
    assert names == sorted(["k_mllt_gsum<%d>" % pb for pb in GSUM] + ["k_mllt_var<%d>" % pb for pb in VAR] + list(SMALL)), names


@pytest.mark.parametrize("pb", sorted(GSUM))
def test_g_instances_have_no_scratch_and_keep_their_budget(notes, pb):
    k = _one(notes, "k_mllt_gsum<%d>" % pb)
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0, k
    vgpr, agpr, lds = GSUM[pb]
    assert k["vgpr"] <= vgpr and k["agpr"] <= agpr and k["lds"] <= lds, k
    # 256 registers a lane still allow two waves a SIMD: the four waves of a workgroup on its four SIMDs, twice
    assert k["vgpr"] + k["agpr"] <= 256, k


@pytest.mark.parametrize("pb", sorted(VAR))
def test_variance_instances_have_no_scratch_and_keep_their_budget(notes, pb):
    k = _one(notes, "k_mllt_var<%d>" % pb)
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0, k
    vgpr, agpr, lds = VAR[pb]
    assert k["vgpr"] <= vgpr and k["agpr"] <= agpr and k["lds"] <= lds, k
    assert k["vgpr"] + k["agpr"] <= 64, k      # eight waves a SIMD


@pytest.mark.parametrize("name", sorted(SMALL))
def test_build_and_adding_kernels(notes, name):
    k = _one(notes, name)
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0, k
    vgpr, agpr, lds = SMALL[name]
    assert k["vgpr"] <= vgpr and k["agpr"] <= agpr and k["lds"] <= lds, k
