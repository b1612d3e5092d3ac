"""What the host decides about the two-launch clipped PPO step (fsrl_amd/csrc/host_decisions.hpp: clip_fuse_update_ok,
clip_fuse_step_ok, clip_fuse_must_replay, clip_fuse_replay_plan) as a stand-alone program: tests/host/clip_fuse_sim.cpp, its own
process, nothing loaded into Python, built with the address / undefined-behaviour sanitizers like tests/test_trust_host.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "clip_fuse_sim.cpp")


def test_selection_rule_and_replay_decision(tmp_path):
    exe = str(tmp_path / "clip_fuse_sim")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-static-libubsan", "-I" + os.path.join(ROOT, "fsrl_amd", "csrc"), SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Sanitizer" not in out.stderr, out.stderr
    oks = [ln for ln in out.stdout.splitlines() if ln.startswith("ok ")]
    assert oks == ["ok update_rule", "ok residency", "ok step_rule", "ok replay"], out.stdout
