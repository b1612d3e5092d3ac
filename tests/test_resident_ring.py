"""The host protocol of the resident actor kernels (fsrl_amd/csrc/resident_ring.hpp) against a kernel made of host threads:
tests/host/resident_ring_sim.cpp, a stand-alone program (its own process, nothing preloaded, nothing loaded into Python), built
with the thread sanitizer and with the address / undefined-behaviour sanitizers.  Its scenarios are the branches no GPU test can
reach -- a stream error while a request is pending, a kernel that never answers, an idle stream without an answer -- next to
the ones the GPU tests do reach (idle timeouts around the calls, release then request, the counters' wrap)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "resident_ring_sim.cpp")


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_resident_ring_protocol_against_a_kernel_of_host_threads(sanitizer, tmp_path):
    exe = str(tmp_path / "resident_ring_sim")
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
    assert out.stdout.count("\nok ") + out.stdout.startswith("ok ") == 7 and "Sanitizer" not in out.stderr, out.stdout + out.stderr
