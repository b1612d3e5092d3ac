"""The plan of fsrl_store_fill (fsrl_amd/csrc/store_fill_plan.hpp) as a stand-alone program: tests/host/store_fill_plan_sim.cpp, its
own process, nothing preloaded, nothing loaded into Python, built with the address / undefined-behaviour sanitizers.  The program
replays random fills against the scalar fsrl_store_push loop the call is defined by: it executes every job table in a random job
order over arrays of row tags, after checking what store_fill_kernel relies on (jobs inside the archive and the store, at most 128
rows, no slot written twice in the launch), and compares the tags, every book and the flag mirror with the loop's."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "store_fill_plan_sim.cpp")


def test_store_fill_plan_equals_the_push_loop(tmp_path):
    exe = str(tmp_path / "store_fill_plan_sim")
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
    assert oks == ["refusals", "cases", "all"], out.stdout
    line = next(ln for ln in out.stdout.splitlines() if ln.startswith("ok cases"))
    f = {k: int(v) for k, v in (kv.split("=") for kv in line.split()[2:])}
    assert f["n"] > 3000
    # cases that wrapped a sub-buffer, cases that left out rows a later row of the same fill overwrites -- and the other ground
    assert f["wrapped"] > 0 and f["dropped"] > 0
    assert f["subsets"] > 0 and f["first_env"] > 0 and f["prewrapped"] > 0
