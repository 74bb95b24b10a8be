"""The weighted-entry scatter kernel's register budget, read from the code object's notes (no GPU needed).

k_scatter_entries<PB> shares its body with k_scatter_items<PB> (tri_scatter_item, tri_scatter.h) and differs in the weight
policy alone: the weight of the entry, read by every thread of the gather so that a row of weight 0 is not fetched.  Wave
R keeps the R + 1 tiles of tile row R in registers for the whole item; a tile that went to scratch memory would be read
and written around every matrix instruction, so every instance must stay free of it, and the LDS of an instance is the
shared body's."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (VGPRs, AGPRs, LDS bytes) of the build this was written with: upper bounds
BUDGET = {1: (72, 8, 5376), 2: (68, 8, 13568), 3: (76, 8, 13568), 4: (88, 8, 21760),
          5: (84, 0, 21760), 6: (92, 0, 29952), 7: (100, 0, 29952), 8: (108, 0, 38144)}
# LDS bytes of k_scatter_items<PB> (tests/test_lda_kernel_notes.py): the body is shared, so these bound the new kernel too
ITEMS_LDS = {1: 5376, 2: 13568, 3: 13568, 4: 21760, 5: 21760, 6: 29952, 7: 29952, 8: 38144}


@pytest.fixture(scope="module")
def notes(capi):
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "scatter_entries.hip.o")
    assert os.path.exists(obj)
    return kernel_notes.kernel_notes(obj)


def test_every_instance_exists_and_nothing_else(notes):
    names = sorted(k.split("::")[-1] for k in notes if "k_scatter" in k)
    assert names == sorted("k_scatter_entries<%d>" % pb for pb in BUDGET), names


@pytest.mark.parametrize("pb", sorted(BUDGET))
def test_entry_instances_have_no_scratch_and_keep_their_budget(notes, pb):
    hits = [v for k, v in notes.items() if k.endswith("k_scatter_entries<%d>" % pb)]
    assert len(hits) == 1, (pb, sorted(notes))
    k = hits[0]
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0, k
    vgpr, agpr, lds = BUDGET[pb]
    assert k["vgpr"] <= vgpr and k["agpr"] <= agpr and k["lds"] <= lds, k
    assert k["lds"] <= ITEMS_LDS[pb], k
    # two workgroups of 64 PB threads a CU at the least: 128 registers a lane would still allow four waves a SIMD
    assert k["vgpr"] + k["agpr"] <= 128, k
