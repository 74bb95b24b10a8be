"""The CMLLR rank-update kernel's register budget, read from the code object's notes (no GPU needed).

k_mllr_rank<PB> keeps a job's accumulator tiles -- PB (PB + 1) / 2 tiles of four doubles a lane -- in registers for a whole
chunk of frames, next to two sets of operands (this step's and the next one's).  A tile that went to scratch memory would
be read and written around every matrix instruction, so every instance must stay free of it."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def notes(capi):
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "mllr_accum.hip.o")
    assert os.path.exists(obj)
    return kernel_notes.kernel_notes(obj)


@pytest.mark.parametrize("pb", [1, 2, 3, 4])
def test_rank_instances_have_no_scratch(notes, pb):
    hits = [v for k, v in notes.items() if k.endswith("k_mllr_rank<%d>" % pb)]
    assert len(hits) == 1, (pb, sorted(notes))
    k = hits[0]
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0, k
    # 48 / 80 / 136 VGPRs and, at <4>, 204 + 80 AGPRs when this was written; 512 is a wave's whole file
    assert k["vgpr"] + k["agpr"] <= 512, k


def test_weight_and_slab_kernels_have_no_scratch(notes):
    for name in ("k_mllr_weights", "k_mllr_slab_add"):
        hits = [v for k, v in notes.items() if name in k]
        assert len(hits) == 1 and hits[0]["scratch"] == 0 and hits[0]["spill_vgpr"] == 0, (name, hits)
