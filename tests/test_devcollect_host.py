"""The decisions and the host replay of a device collect (fsrl_amd/csrc/devcollect_plan.hpp) as a stand-alone program:
tests/host/devcollect_sim.cpp, its own process, nothing preloaded, nothing loaded into Python, built with the address / undefined-
behaviour sanitizers.  The surplus rule is held against a brute-force restatement of fsrl/data/fast_collector.py:341-362 for every
(env_num <= 6, n_episode <= 8, pattern of episode ends over 4 vector steps); the replay of a log of rows against direct bookkeeping
on sub-buffers that wrap."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "devcollect_sim.cpp")


def test_devcollect_decisions_and_replay(tmp_path):
    exe = str(tmp_path / "devcollect_sim")
    # -static-lib*san: a dynamically linked sanitizer runtime must be the first library loaded (tests/test_train_state_host.py)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "fsrl_amd", "csrc"), SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    oks = [ln.split()[1] for ln in out.stdout.splitlines() if ln.startswith("ok ")]
    assert oks == ["limits", "surplus", "replay", "all"], out.stdout
    f = dict(kv.split("=") for kv in next(ln for ln in out.stdout.splitlines() if ln.startswith("ok surplus")).split()[2:])
    assert int(f["cases"]) > 100000 and int(f["dropped"]) > 0 and int(f["finished"]) > 0
