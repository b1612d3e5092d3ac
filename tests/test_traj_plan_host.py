"""The trajectory archive's bookkeeping and job planning (fsrl_amd/csrc/traj_plan.hpp) as a stand-alone program:
tests/host/traj_plan_sim.cpp, its own process, nothing preloaded, nothing loaded into Python, built with the address / undefined-
behaviour sanitizers.  The program models the device by arrays of row tags and executes every job table in a random job order, after
checking what traj_move_kernel relies on: jobs inside their buffers, source and destination different memory, no row written twice
in a launch; after every step every alive row is where the episode table says, once."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "traj_plan_sim.cpp")


def test_traj_plan_places_every_alive_row_once(tmp_path):
    exe = str(tmp_path / "traj_plan_sim")
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
    assert oks == ["window_and_limits", "run", "run", "run", "all"], out.stdout
    for ln in out.stdout.splitlines():
        if ln.startswith("ok run"):
            f = dict(kv.split("=") for kv in ln.split()[2:])
            # every run exercised commits, refusals for lack of room, compactions, keeps and replacements
            assert all(int(f[k]) > 0 for k in ("committed", "refused", "compactions", "keeps", "replaced")), ln
