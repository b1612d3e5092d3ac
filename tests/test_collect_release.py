"""The release hook of a collect group under threads (fsrl_amd/csrc/resident_ring.hpp: rr_release_guarded, which
collect_group_actor_release runs): tests/host/collect_release_sim.cpp, a stand-alone program (its own process, nothing preloaded,
nothing loaded into Python) -- 8 threads hammer the hook against a kernel made of host threads while the main thread alternates
request and release -- built with the thread sanitizer and with the address / undefined-behaviour sanitizers.  It passes when it
exits 0: exactly one EXIT per live generation, `seq` never repeats.  Built with -DUNGUARDED (the hook before the mutex) the thread
sanitizer reports the race; that build is not part of the test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "collect_release_sim.cpp")


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_release_hook_from_eight_threads_against_a_kernel_of_host_threads(sanitizer, tmp_path):
    exe = str(tmp_path / "collect_release_sim")
    # -static-lib*san: a sanitizer runtime that is linked dynamically refuses to start unless it is the first library the process
    # loads, so the program would not run where the environment preloads any library of its own.  Linked in, it starts anywhere.
    static = ["-static-libtsan"] if sanitizer == "thread" else ["-static-libasan", "-static-libubsan"]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=" + sanitizer, "-fno-sanitize-recover=undefined", *static,
           "-I" + os.path.join(ROOT, "fsrl_amd", "csrc"), SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok  one EXIT per live generation, seq never repeats" in out.stdout and "Sanitizer" not in out.stderr, out.stdout + out.stderr
