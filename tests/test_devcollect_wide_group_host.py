"""Grouped wide device collects without a GPU: the registers of every grouped wide kernel instantiation in the gfx950 code object
(tools/sonotes.py, as tests/test_devcollect_wide_host.py reads the solo kernels'), and the block -> (member, tile) mapping of
fsrl_amd/csrc/devcollect_plan.hpp as a stand-alone program built with the address / undefined-behaviour sanitizers."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "fsrl_amd", "libfsrl_hip.so")


def test_grouped_wide_kernel_instantiations_do_not_spill():
    """fused: H = 64 / 128 / 256 x both envs x the three heads; layered: both envs x the three heads x (LDS, workspace): zero spilled
    registers, no scratch, at most 128 VGPRs"""
    assert os.path.exists(LIB), "libfsrl_hip.so is not built"
    import sonotes
    pat = re.compile(r"^_Z\d+wide_(collect|layered)_group_step_kernelI(?:Li(\d+)E)?\d+DevEnv[A-Za-z]+Li\dE")
    seen = {}
    for name, k in sonotes.kernel_notes(LIB).items():
        m = pat.match(name)
        if m:
            seen[m.group(1), m.group(2)] = seen.get((m.group(1), m.group(2)), 0) + 1
            assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (name, k)
            assert k["vgpr_count"] <= 128, (name, k)
    assert seen == {("collect", "64"): 6, ("collect", "128"): 6, ("collect", "256"): 6, ("layered", None): 12}, seen


def test_block_to_member_and_tile_mapping(tmp_path):
    exe = str(tmp_path / "devcollect_wide_group_sim")
    # -static-lib*san: a dynamically linked sanitizer runtime must be the first library loaded (tests/test_train_state_host.py)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-static-libubsan", "-I" + os.path.join(ROOT, "fsrl_amd", "csrc"), os.path.join(ROOT, "tests", "host", "devcollect_wide_group_sim.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.endswith("ok all\n") and "runtime error" not in out.stderr, out.stdout + out.stderr
