"""The full-statistics kernels' register and memory budget, read from the code object's notes (no GPU needed).

k_full_units<PB> is k_scatter_items' shape with the weight read from the unit's posteriors: wave R of a workgroup holds
the R + 1 tiles of tile row R in registers for the whole unit -- eight tiles of four doubles a lane at PB = 8 -- beside the
eight values a thread carries from global memory to LDS.  A tile in scratch memory would be read and written around every
matrix instruction, so every instance must stay free of it.  This reads register and memory notes only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (VGPRs, AGPRs, LDS bytes) of the build this was written with: upper bounds
BUDGET = {1: (72, 8, 5376), 2: (68, 8, 13568), 3: (76, 8, 13568), 4: (88, 8, 21760),
          5: (84, 0, 21760), 6: (92, 0, 29952), 7: (100, 0, 29952), 8: (108, 0, 38144)}
OTHERS = {"k_full_lik": 12, "k_full_norm": 16, "k_full_slab_add": 8, "k_full_pack": 11}     # VGPRs; no LDS


@pytest.fixture(scope="module")
def notes(capi):
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "stats_full_accum.hip.o")
    assert os.path.exists(obj)
    return kernel_notes.kernel_notes(obj)


def test_every_full_kernel_is_covered(notes):
    names = sorted(k.split("::")[-1] for k in notes if "k_full" in k)
    assert names == sorted(["k_full_units<%d>" % pb for pb in BUDGET] + list(OTHERS)), names


@pytest.mark.parametrize("pb", sorted(BUDGET))
def test_unit_instances_have_no_scratch_and_keep_their_budget(notes, pb):
    hits = [v for k, v in notes.items() if k.endswith("k_full_units<%d>" % pb)]
    assert len(hits) == 1, (pb, sorted(notes))
    k = hits[0]
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0, k
    vgpr, agpr, lds = BUDGET[pb]
    assert k["vgpr"] <= vgpr and k["agpr"] <= agpr and k["lds"] <= lds, k
    # two workgroups of 64 PB threads a CU at the least: 128 registers a lane would still allow four waves a SIMD
    assert k["vgpr"] + k["agpr"] <= 128, k


@pytest.mark.parametrize("name", sorted(OTHERS))
def test_the_other_kernels_have_no_scratch(notes, name):
    hits = [v for k, v in notes.items() if k.split("::")[-1] == name]
    assert len(hits) == 1, sorted(notes)
    k = hits[0]
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0 and k["lds"] == 0, k
    assert k["vgpr"] <= OTHERS[name] and k["agpr"] == 0, k
