"""The owner of device and pinned memory (fsrl_amd/csrc/dev_mem.hpp: dev / pinned / release / regrow / release_all) over a checking
malloc backend, as a stand-alone program: tests/host/dev_mem_sim.cpp, its own process, nothing loaded into Python, built with the
address / undefined-behaviour sanitizers like tests/test_clip_fuse_host.py.  regrow_fails is the case the hand-kept regrows got
wrong: an allocation fails, and the next call needs less than the old capacity."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "dev_mem_sim.cpp")


def test_owner_frees_everything_once_and_regrow_survives_a_failed_allocation(tmp_path):
    exe = str(tmp_path / "dev_mem_sim")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-static-libubsan", "-I" + os.path.join(ROOT, "fsrl_amd", "csrc"), SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Sanitizer" not in out.stderr, out.stderr
    oks = [ln for ln in out.stdout.splitlines() if ln.startswith("ok ")]
    assert oks == ["ok release_all", "ok release", "ok regrow", "ok regrow_fails", "ok reuse"], out.stdout
