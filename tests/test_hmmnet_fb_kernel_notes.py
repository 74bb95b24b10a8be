"""The forward-backward kernel's memory budget, read from the code object's notes (no GPU needed).

csrc/hmmnet_fb.h states the layout: the LDS form holds two node vectors of FB_LDS_NODES = 2048 doubles (32 KB) and the
256-double reduction pad (2 KB), the global form the pad (and one placeholder double) only.  Neither form may touch
scratch memory: a lane's state is a handful of doubles, and a private array or a spilled vector register would sit
inside the per-frame loops.  (The kernel is three phases in one body and its scalar registers are full; the compiler
parks some scalars in vector-register lanes, which is no memory traffic -- spill_vgpr and scratch are what is pinned.)"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FB_THREADS, FB_LDS_NODES = 256, 2048
LDS = {"k_hmmnet_fb<true>": (2 * FB_LDS_NODES + FB_THREADS) * 8, "k_hmmnet_fb<false>": (1 + FB_THREADS) * 8}


@pytest.fixture(scope="module")
def notes(capi):
    import kernel_notes
    obj = os.path.join(ROOT, "aaltoasr_amd", "lib", "obj", "hmmnet_fb.hip.o")
    assert os.path.exists(obj)
    return kernel_notes.kernel_notes(obj)


def test_the_name_set(notes):
    assert sorted(k.split("::")[-1] for k in notes) == sorted(LDS), sorted(notes)


def test_the_header_states_these_sizes():
    text = open(os.path.join(ROOT, "aaltoasr_amd", "csrc", "hmmnet_fb.h")).read()
    assert "FB_THREADS = %d" % FB_THREADS in text and "FB_LDS_NODES = %d" % FB_LDS_NODES in text


@pytest.mark.parametrize("name", sorted(LDS))
def test_no_scratch_and_lds_within_the_header(notes, name):
    k = [v for n, v in notes.items() if n.split("::")[-1] == name][0]
    assert k["scratch"] == 0 and k["spill_vgpr"] == 0, k
    assert k["lds"] <= LDS[name], k
    # four utterances a CU in the LDS form (4 x 34 KB of 160 KB): 256 lanes x 128 registers each leave room for them
    assert k["vgpr"] + k["agpr"] <= 128, k
