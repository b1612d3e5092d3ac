"""The bookkeeping of a lock-step collect of k members over worker-process envs (fsrl_amd/csrc/group_episodes.hpp, the loop of
fsrl_group_collect_episodes / fsrl_collect_episodes_group) without a GPU: tests/host/group_episodes_sim.cpp, a stand-alone program
(its own process, nothing preloaded, nothing loaded into Python) built with the address / undefined-behaviour sanitizers.  It
drives the header with fake envs -- observation, reward, cost and done a function of (member, env, time), the reward also of the
action found in the env's slot -- and a fake step call that records what every member is asked to store and to act on, and compares
each member's record with a single-member collect loop the program writes out on its own (FastCollector's rule: reset the finished
envs, drop the first `surplus` of them, stop at n_episode).  Cases: k = 3 with episode lengths 5 / 7 / 4, env counts 17 / 3 / 4 and
n_episode 20 / 6 / 2 (more episodes than envs, surplus envs dropped, fewer episodes than envs), the same with episodes that end in
different steps, k = 1, a member whose episodes all end in the same step, an env command that fails at step 3 for member 1 (no
further step call, member 1 named), and the argument refusals.  k = 1 is fsrl_collect_episodes' own loop.

The split loop (ge_collect_split, the loop of fsrl_collect_episodes_split) runs in the same program against a two-lane loop written
out the way FastCollector._collect_split has it; a posted command takes effect only when its lane is waited for, and every request,
post (lane, command, env ids) and wait is compared in order.  Do = 5, Da = 2; six envs of episode length 19: 3 + 3 on the lanes with
n_episode 6, 10, 3, 1, 7, 12 back to back; 5 + 1; all ready envs on lane 0; episodes that end in different steps on the two lanes;
both lanes finishing in one round with fewer episodes wanted than finished; fewer episodes than envs (one trailing wait for the lane
still stepping); a wait that fails on lane 1 at its third step (lane 0 reported busy, no further post or step call); the refusals."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "group_episodes_sim.cpp")


def test_every_members_requests_under_the_group_equal_its_own_collects(tmp_path):
    exe = str(tmp_path / "group_episodes_sim")
    # -static-lib*san: a sanitizer runtime that is linked dynamically refuses to start unless it is the first library the process
    # loads; linked in, the program starts anywhere (as tests/test_collect_release.py builds its program)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-static-libubsan", "-I" + os.path.join(ROOT, "fsrl_amd", "csrc"), SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
    for case in ("k3:", "k3 staggered:", "k1:", "one member's episodes all end in the same step:", "env failure:", "refusals:",
                 "split basic:", "split uneven lanes:", "split one lane empty:", "split staggered:", "split both lanes in one round:",
                 "split fewer episodes than envs:", "split failing wait:", "split refusals:", "all"):
        assert "ok  " + case in out.stdout, out.stdout


def test_the_header_uses_no_hip_and_no_context():
    src = open(os.path.join(ROOT, "fsrl_amd", "csrc", "group_episodes.hpp")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "hip" not in code.lower() and "fsrl_ctx" not in code
    glue = open(os.path.join(ROOT, "fsrl_amd", "csrc", "host_group_episodes.inc")).read()
    assert '#include "group_episodes.hpp"' in glue and "ge_collect(" in glue
    solo = open(os.path.join(ROOT, "fsrl_amd", "csrc", "host_collect.inc")).read()
    assert '#include "group_episodes.hpp"' in solo and "ge_collect(" in solo and "ge_collect_split(" in solo
