"""The blocked-moments kernels' register budget, read from the code object's notes (no GPU needed).

k_moments_full<PB> gives wave R of a workgroup the R + 1 tiles of tile row R, as k_scatter_items does, and reads its
operands straight from global memory into registers: R + 1 operand values a lane beside the tiles, no LDS at all.  A
tile that went to scratch memory would be read and written around every matrix instruction, so every instance must stay
free of it -- also the select that picks the wave's A operand out of its B operands, which indexes registers by the
wave's row and must not become an indexed array in scratch.  k_moments_diag keeps two sums a thread and two LDS arrays
of 256 doubles."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (VGPRs, AGPRs, LDS bytes) of the build this was written with: upper bounds
BUDGET = {1: (28, 8, 0), 2: (40, 8, 0), 3: (48, 8, 0), 4: (60, 8, 0),
          5: (59, 0, 0), 6: (69, 0, 0), 7: (79, 0, 0), 8: (89, 0, 0)}
DIAG = (42, 0, 4096)


@pytest.fixture(scope="module")
def notes(capi):
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "moments_accum.hip.o")
    assert os.path.exists(obj)
    return kernel_notes.kernel_notes(obj)


def test_every_moments_kernel_is_covered(notes):
    names = sorted(k.split("::")[-1] for k in notes if "k_moments" in k)
    assert names == sorted(["k_moments_full<%d>" % pb for pb in BUDGET] + ["k_moments_diag", "k_moments_seg_add"]), names


@pytest.mark.parametrize("pb", sorted(BUDGET))
def test_full_instances_have_no_scratch_and_keep_their_budget(notes, pb):
    hits = [v for k, v in notes.items() if k.endswith("k_moments_full<%d>" % pb)]
    assert len(hits) == 1, (pb, sorted(notes))
    k = hits[0]
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0, k
    vgpr, agpr, lds = BUDGET[pb]
    assert k["vgpr"] <= vgpr and k["agpr"] <= agpr and k["lds"] <= lds, k
    # 128 registers a lane still allow four waves a SIMD
    assert k["vgpr"] + k["agpr"] <= 128, k


def test_diagonal_and_adding_kernels(notes):
    hits = [v for k, v in notes.items() if "k_moments_diag" in k]
    assert len(hits) == 1, sorted(notes)
    k = hits[0]
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["spill_sgpr"] == 0, k
    assert k["vgpr"] <= DIAG[0] and k["agpr"] <= DIAG[1] and k["lds"] <= DIAG[2], k
    hits = [v for k, v in notes.items() if "k_moments_seg_add" in k]
    assert len(hits) == 1 and hits[0]["scratch"] == 0 and hits[0]["spill_vgpr"] == 0, hits
