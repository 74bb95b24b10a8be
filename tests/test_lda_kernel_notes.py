"""The class-scatter kernel's register budget, read from the code object's notes (no GPU needed).

k_scatter_items<PB> gives wave R of a workgroup the R + 1 tiles of tile row R -- at most eight tiles of four doubles a
lane at PB = 8, where one wave could not hold all 36 -- and keeps them in registers for the whole item, beside the eight
values a thread carries from global memory to LDS.  A tile that went to scratch memory would be read and written around
every matrix instruction, so every instance must stay free of it."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (VGPRs, AGPRs, LDS bytes) of the build this was written with: upper bounds
BUDGET = {1: (72, 8, 5376), 2: (68, 8, 13568), 3: (76, 8, 13568), 4: (88, 8, 21760),
          5: (82, 0, 21760), 6: (90, 0, 29952), 7: (98, 0, 29952), 8: (106, 0, 38144)}


@pytest.fixture(scope="module")
def notes(capi):
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "scatter_accum.hip.o")
    assert os.path.exists(obj)
    return kernel_notes.kernel_notes(obj)


def test_every_scatter_kernel_is_covered(notes):
    names = sorted(k.split("::")[-1] for k in notes if "k_scatter" in k)
    assert names == sorted(["k_scatter_items<%d>" % pb for pb in BUDGET] + ["k_scatter_slab_add"]), names


@pytest.mark.parametrize("pb", sorted(BUDGET))
def test_item_instances_have_no_scratch_and_keep_their_budget(notes, pb):
    hits = [v for k, v in notes.items() if k.endswith("k_scatter_items<%d>" % pb)]
    assert len(hits) == 1, (pb, sorted(notes))
    k = hits[0]
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0, k
    vgpr, agpr, lds = BUDGET[pb]
    assert k["vgpr"] <= vgpr and k["agpr"] <= agpr and k["lds"] <= lds, k
    # two workgroups of 64 PB threads a CU at the least: 128 registers a lane would still allow four waves a SIMD
    assert k["vgpr"] + k["agpr"] <= 128, k


def test_slab_kernel_has_no_scratch(notes):
    hits = [v for k, v in notes.items() if "k_scatter_slab_add" in k]
    assert len(hits) == 1 and hits[0]["scratch"] == 0 and hits[0]["spill_vgpr"] == 0, hits
