"""The host-side decisions at the edges of a PPO update (fsrl_amd/csrc/host_decisions.hpp): the layout of fsrl_ppo_begin's one packed
upload (fixed head, 64-byte starts, no overlap, inside the capacity allocated for the store), the split of process_fn's workgroups
between the full jobs and the jobs that walk the listed V(obs_next) rows (never more workgroups than the launch has, full jobs never
below the equal split, the equal split exactly when no rows coincide), and the host count of coinciding rows (words, not floats).
tests/host/update_edges_sim.cpp is a plain program: its own process, nothing loaded into Python, built with the address /
undefined-behaviour sanitizers.  The kernel calls the same infer_split (the header is compiled for the device too), and
tests/test_gpu_ppo_vnext_reuse.py checks the counters it leads to on the device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "update_edges_sim.cpp")


def test_upload_layout_and_infer_split(tmp_path):
    exe = str(tmp_path / "update_edges_sim")
    # -static-lib*san: see tests/test_resident_ring.py (a dynamically linked sanitizer runtime must be the first library loaded)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-static-libubsan", "-I" + os.path.join(ROOT, "fsrl_amd", "csrc"), SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    oks = [ln for ln in out.stdout.splitlines() if ln.startswith("ok ")]
    assert len(oks) == 3 and "Sanitizer" not in out.stderr, out.stdout + out.stderr
    assert oks[0].startswith("ok upload_layout cases=") and int(oks[0].split("cases=")[1]) >= 100
    assert oks[1].startswith("ok infer_split cases=") and oks[1].endswith("headline=1/84")
    assert oks[2] == "ok next_same_count"
