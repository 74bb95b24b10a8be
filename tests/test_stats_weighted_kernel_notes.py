"""The memory budget of the weighted accumulation kernel and of the entry kernels, read from the code objects' notes
(no GPU needed).

csrc/stats_weighted.hip: k_stats_items_w is k_stats_items (stats_accum.hip) with a weight per entry -- the same ten
dimension instances, no LDS of its own beyond the launch's dynamic one.  Up to <128> a lane's frame fits its
registers: no scratch memory and no spilled vector register (the plain kernel's <192> spills already, and so does
this one; it runs, slowly, for pools of 129 ... 192 dimensions).  The instances that production feature dimensions
use, <24> ... <48>, are pinned at the vector registers measured on this build -- 113, 129, 145 and 162, two more
than the plain kernel's 111, 127, 143 and 160 (the weight is a double), all within the 168 that keep three waves a
SIMD -- as "does not grow".

csrc/fb_entries.hip: three kernels of a few registers, no scratch, no LDS."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

INSTANCES = (8, 16, 24, 32, 40, 48, 64, 96, 128, 192)
MEASURED_VGPR = {24: 113, 32: 129, 40: 145, 48: 162}
ENTRY_KERNELS = ("k_fb_entry_counts", "k_fb_entry_fill", "k_fb_frame_sums")


def _notes(name):
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", name)
    assert os.path.exists(obj), obj
    return {k.split("::")[-1]: v for k, v in kernel_notes.kernel_notes(obj).items()}


@pytest.fixture(scope="module")
def weighted(capi):
    return _notes("stats_weighted.hip.o")


@pytest.fixture(scope="module")
def entry(capi):
    return _notes("fb_entries.hip.o")


def test_the_name_sets(weighted, entry):
    assert sorted(weighted) == sorted("k_stats_items_w<%d>" % n for n in INSTANCES), sorted(weighted)
    assert sorted(entry) == sorted(ENTRY_KERNELS), sorted(entry)


@pytest.mark.parametrize("n", [n for n in INSTANCES if n <= 128])
def test_no_scratch_up_to_128_dimensions(weighted, n):
    k = weighted["k_stats_items_w<%d>" % n]
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0, k


@pytest.mark.parametrize("n", sorted(MEASURED_VGPR))
def test_production_instances_do_not_grow(weighted, n):
    k = weighted["k_stats_items_w<%d>" % n]
    assert k["vgpr"] <= MEASURED_VGPR[n] <= 168 and k["agpr"] == 0, k


@pytest.mark.parametrize("name", ENTRY_KERNELS)
def test_entry_kernels_are_small(entry, name):
    k = entry[name]
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["lds"] == 0 and k["vgpr"] <= 32, k
