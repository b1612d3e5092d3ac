"""The fused PPO kernel family in the built library's gfx950 code object, read on the host (no GPU; tools/sonotes.py as in
test_code_object.py): every `ppo_fwd_bwd_kernel<H, R, early>` instantiation -- the one-burst ones and the ones that issue the
backward W2 fragment from inside the forward pass (kernels_mlp.hpp: W2bEarly) -- has zero spilled VGPRs, zero bytes of scratch and at
most 128 VGPRs (what 1024 threads per workgroup allow), and both instantiations of the 4- and 8-row tiles exist at every width, so
that a context created under FSRL_NO_W2B_EARLY has a different kernel to launch (tests/test_gpu_ppo_w2b_early.py compares the two)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")
PREFIX = "_Z18ppo_fwd_bwd_kernelILi"


@pytest.fixture(scope="module")
def family():
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    import sonotes
    fam = {n: k for n, k in sonotes.kernel_notes(LIB).items() if n.startswith(PREFIX)}
    assert fam, "no ppo_fwd_bwd_kernel in the code object's metadata note"
    return fam


def test_both_instantiations_of_the_short_tiles_exist_at_every_width(family):
    for H in (64, 128, 256):
        for R in (4, 8):
            for early in (0, 1):
                want = "%s%dELi%dELb%dEE" % (PREFIX, H, R, early)
                assert any(n.startswith(want) for n in family), want
        assert any(n.startswith("%s%dELi16ELb0EE" % (PREFIX, H)) for n in family), H
        assert not any(n.startswith("%s%dELi16ELb1EE" % (PREFIX, H)) for n in family), H      # 16-row tiles keep the one burst


def test_the_shipped_library_reads_the_switch():
    """the getenv name is in the product's host code only if the read is compiled into it (not inside the probe-only block)"""
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    with open(LIB, "rb") as f:
        assert b"FSRL_NO_W2B_EARLY\0" in f.read()


def test_no_spill_no_scratch_and_the_register_budget_of_1024_threads(family):
    for name, k in family.items():
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)
