"""The log-likelihood kernel's register and memory budget, read from the code object's notes (no GPU needed).

k_segll_items keeps a lane's four running sums, its row operand and the exp / log evaluation in registers and takes
the mixture's records through the scalar cache; its only LDS is the dynamic tile of rows that the host sizes (at most
64 KB, tests/test_segll_gpu.py), so the static figure is 0.  Scratch memory or a spilled register would sit inside the
loop over components and dimensions.  The figures are those of the build this was written with, as upper bounds."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

BUDGET = {"k_segll_items": (66, 0, 0)}     # VGPRs, AGPRs, static LDS bytes


@pytest.fixture(scope="module")
def notes(capi):
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "seg_loglik.hip.o")
    assert os.path.exists(obj)
    return kernel_notes.kernel_notes(obj)


def test_the_name_set(notes):
    assert sorted(k.split("::")[-1] for k in notes) == sorted(BUDGET), sorted(notes)


@pytest.mark.parametrize("name", sorted(BUDGET))
def test_no_scratch_no_spills_and_the_budget(notes, name):
    k = [v for n, v in notes.items() if n.split("::")[-1] == name][0]
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0, k
    vgpr, agpr, lds = BUDGET[name]
    assert k["vgpr"] <= vgpr and k["agpr"] <= agpr and k["lds"] <= lds, k
    # 256 lanes a workgroup and two workgroups a CU (their LDS tiles): 128 registers a lane leave room for both
    assert k["vgpr"] + k["agpr"] <= 128, k
