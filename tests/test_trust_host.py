"""What the trust-region updates decide on the host between their launches (fsrl_amd/csrc/host_decisions.hpp: CPO's dual solve, the
line searches' schedules and acceptance rules, the minibatch split, the permutation check / shuffle, the tile-split simulation)
as a stand-alone program: tests/host/trust_host_sim.cpp, its own process, nothing preloaded, nothing loaded into Python, built with
the address / undefined-behaviour sanitizers and WITHOUT -march / -ffast-math (the library's host code is baseline x86-64 too, so
both run the same arithmetic).  This side reads the fixtures recorded from the unmodified reference and hands their rows over as
text; the program reads no fixture format."""
import glob
import json
import os
import subprocess

import numpy as np

from helpers import GOLDEN, load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "trust_host_sim.cpp")


def _rows():
    """-> (dual rows, schedule rows): every row of stats_actor of tests/golden/cpo_*.npz, plus pl_stats of cpo_perturbed.npz"""
    dual, sched = [], []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "cpo_*.npz"))):
        g = load_npz(os.path.basename(path))
        cfg = json.loads(str(g["cfg_json"]))
        tables = []
        if "stats_actor" in g:
            tables.append(([str(k) for k in g["stats_actor_keys"]], np.atleast_2d(g["stats_actor"]), True))
        if "pl_stats" in g:
            tables.append(([str(k) for k in g["pl_stats_keys"]], np.atleast_2d(g["pl_stats"]), False))
        for keys, table, with_sched in tables:
            for row in table:
                v = {k.split("/")[1]: float(np.float32(row[keys.index(k)])) for k in keys}
                case = int(v["optim_case"])
                dual.append((v["optim_Q"], v["optim_R"], v["optim_S"], v["optim_C"], float(np.float32(cfg.get("target_kl", 0.01))),
                             0.0 if case == 4 else 1.0,                  # b.b is not recorded: 0 where the reference took case 4
                             case, v["optim_A"], v["optim_B"], v["optim_lam"], v["optim_nu"]))
                if with_sched:
                    sched.append((v["step_size"], float(cfg["backtrack_coeff"]), int(cfg["max_backtracks"])))
    return dual, sched


def test_host_decisions_against_the_reference_rows_and_scripted_cases(tmp_path):
    """Worst relative error of A, B, lam, nu over the 31 recorded dual solves, as the program prints it: 1.001e-07 (under one
    float32 ulp; the bar, asserted by the program, is two: 2.384e-07).  Every recorded optim_case is reproduced exactly."""
    dual, sched = _rows()
    assert len(dual) == 31 and len(sched) == 30
    counts = [sum(1 for d in dual if d[6] == c) for c in range(5)]
    assert min(counts) >= 2, counts                                      # every branch of the solve, at least twice: 18 / 2 / 2 / 7 / 2
    rows = tmp_path / "rows.txt"
    with open(rows, "w") as f:
        for d in dual:
            f.write("dual " + " ".join(repr(x) for x in d) + "\n")
        for s in sched:
            f.write("sched " + " ".join(repr(x) for x in s) + "\n")
    exe = str(tmp_path / "trust_host_sim")
    # -static-lib*san: see tests/test_resident_ring.py (a dynamically linked sanitizer runtime must be the first library loaded)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-static-libubsan", "-I" + os.path.join(ROOT, "fsrl_amd", "csrc"), SRC, "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe, str(rows)], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    oks = [ln for ln in out.stdout.splitlines() if ln.startswith("ok ")]
    assert len(oks) == 8 and "Sanitizer" not in out.stderr, out.stdout + out.stderr
    assert oks[0].startswith("ok dual_recorded rows=31 cases=%d/%d/%d/%d/%d " % tuple(counts)), oks[0]
    assert oks[1] == "ok sched_recorded rows=30", oks[1]
    assert float(oks[0].split("worst_rel=")[1]) <= 2.0 * 2.0 ** -23
