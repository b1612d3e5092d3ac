"""Microseconds per behaviour-cloning update (fsrl_bc_update) next to the same regression in stock torch (torch.nn + torch.optim.Adam)
on the same GPU.  Shapes: 256 x 256, obs 33 / act 8, batch 256 and 1024; 64 x 64, obs 6 / act 2, batch 256.  Every window is UPDATES
(torch) or HIP_UPDATES (fsrl_bc_update: windows of a few hundred ms) updates and ends in a device synchronise; the HIP window includes
the host's draw of its batch x updates indices, torch draws on the device; the two paths alternate, ROUNDS rounds after a warm-up window of each; median and min - max.
    python tools/bench_bc.py [--out profiles/bc_update.json]
--ks 1,2,4,8: k seeds pre-trained at once instead (fsrl_bc_update_group), microseconds per MEMBER update in three modes that alternate
within a round: `grouped` (one bc_update_group call, each member GROUP_UPDATES updates from its own store and seed), `in_turn` (k solo
bc_update calls one after the other) and `threads` (k threads, a solo call each).  --ab-tree PATH adds `solo_ab`: the solo update of
this tree and of the built checkout of another commit at PATH (its package and library), a fresh process per window, the two alternating.
    python tools/bench_bc.py --ks 1,2,4,8 [--ab-tree /path/to/built/checkout] --out profiles/bc_update_group.json
--hidden 64x48x32,256x256x256,1024x1024: these hidden_sizes instead (obs 33 / act 8, batch 256), each through the call its shape routes to
(a layered shape: fsrl_bc_update_layered, windows of UPDATES updates) next to the same stock-torch loop over a network of that depth.
    python tools/bench_bc.py --hidden 64x48x32,256x256x256,1024x1024 --out profiles/bc_update_layered.json
"""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.environ.get("FSRL_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # --ab-tree's children
from fsrl_amd.engine import Engine, EngineConfig
from fsrl_amd.data.device_collector import _layered

SHAPES = [((256, 256), 33, 8, 256), ((256, 256), 33, 8, 1024), ((64, 64), 6, 2, 256)]
ROWS, UPDATES, HIP_UPDATES, ROUNDS = 4096, 2000, 10000, 7
GROUP_UPDATES = 2500


def hip_window(hidden, Do, Da, B, rng):
    eng = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden_sizes=hidden, env_num=16, buffer_size=ROWS), device=0)
    eng.set_params((0.1 * rng.standard_normal(eng.n_params)).astype(np.float32))
    ids, z, f = np.arange(16), np.zeros(16), np.zeros(16, bool)
    for _ in range(ROWS // 16):
        o = rng.standard_normal((16, Do)).astype(np.float32)
        eng.push(ids, o, np.tanh(rng.standard_normal((16, Da))).astype(np.float32), z, z, f, f, o)
    if _layered(eng):
        return eng, lambda n=UPDATES: eng.bc_update_layered(B, n, loss="mse", seed=1)
    return eng, lambda n=HIP_UPDATES: eng.bc_update(B, n, loss="mse", seed=1)      # returns the losses: synchronises


def torch_window(hidden, Do, Da, B, rng):
    dev = torch.device("cuda:0")
    widths = [Do, *hidden]
    body = [m for i, o in zip(widths, widths[1:]) for m in (torch.nn.Linear(i, o), torch.nn.ReLU())]
    net = torch.nn.Sequential(*body, torch.nn.Linear(widths[-1], Da), torch.nn.Tanh()).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    obs = torch.tensor(rng.standard_normal((ROWS, Do)), dtype=torch.float32, device=dev)
    act = torch.tanh(torch.tensor(rng.standard_normal((ROWS, Da)), dtype=torch.float32, device=dev))

    def run():
        for _ in range(UPDATES):
            idx = torch.randint(0, ROWS, (B,), device=dev)
            loss = ((net(obs[idx]) - act[idx]) ** 2).sum(1).mean()
            opt.zero_grad(set_to_none=True); loss.backward(); opt.step()
        torch.cuda.synchronize()
    return None, run


def spread(row, name, v):
    row[name + "_us_median"], row[name + "_us_min"], row[name + "_us_max"] = float(np.median(v)), min(v), max(v)


def group_rows(ks):
    """one row per (shape, k): us per member update, grouped | k solo calls in turn | k threads of solo calls"""
    from fsrl_amd.engine import bc_update_group
    n = GROUP_UPDATES
    for hidden, Do, Da, B in SHAPES:
        rng = np.random.default_rng(0)
        members = [hip_window(hidden, Do, Da, B, rng) for _ in range(max(ks))]
        for k in ks:
            engs, solo = [e for e, _ in members[:k]], [f for _, f in members[:k]]

            def threads():
                ts = [threading.Thread(target=f, args=(n,)) for f in solo]
                [t.start() for t in ts]; [t.join() for t in ts]
            modes = (("grouped", lambda: bc_update_group(engs, B, n, loss="mse", seeds=1)), ("in_turn", lambda: [f(n) for f in solo]),
                     ("threads", threads))
            us = {name: [] for name, _ in modes}
            for r in range(ROUNDS + 1):          # round 0 warms every mode up
                for name, fn in modes:
                    t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
                    if r:
                        us[name].append(dt * 1e6 / (k * n))
            row = {"hidden": list(hidden), "obs_dim": Do, "act_dim": Da, "batch": B, "k": k, "updates_per_member_per_window": n, "rounds": ROUNDS}
            for name, v in us.items():
                spread(row, name, v)
            print(json.dumps(row), flush=True)
            yield row
        for e, _ in members:
            e.close()


def solo_window():
    """--solo-window (a child of --ab-tree): one window of the solo update per shape with the package of the tree FSRL_BENCH_TREE names"""
    out = []
    for hidden, Do, Da, B in SHAPES:
        eng, hip = hip_window(hidden, Do, Da, B, np.random.default_rng(0))
        hip(GROUP_UPDATES)
        t0 = time.perf_counter(); hip(); out.append((time.perf_counter() - t0) * 1e6 / HIP_UPDATES)
        eng.close()
    print("SOLO " + json.dumps(out))


def solo_ab(other):
    us = {"this_build": [], "other_build": []}
    for _ in range(ROUNDS):
        for name, tree in (("this_build", None), ("other_build", other)):
            env = dict(os.environ)
            env.pop("FSRL_BENCH_TREE", None)
            if tree:
                env["FSRL_BENCH_TREE"] = os.path.abspath(tree)
            txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--solo-window"], env=env, capture_output=True, text=True, check=True).stdout
            us[name].append(json.loads([ln for ln in txt.splitlines() if ln.startswith("SOLO ")][-1][5:]))
    rows = []
    for j, (hidden, Do, Da, B) in enumerate(SHAPES):
        row = {"hidden": list(hidden), "obs_dim": Do, "act_dim": Da, "batch": B, "updates_per_window": HIP_UPDATES, "rounds": ROUNDS}
        for name, v in us.items():
            spread(row, name, [w[j] for w in v])
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ks", default=None, type=lambda t: [int(v) for v in t.split(",")], help="group sizes, e.g. 1,2,4,8: measure fsrl_bc_update_group")
    ap.add_argument("--ab-tree", default=None, help="with --ks: a built checkout of another commit, its solo update alternated with this tree's")
    ap.add_argument("--hidden", default=None, type=lambda t: [tuple(int(w) for w in h.split("x")) for h in t.split(",")],
                    help="hidden_sizes tuples, e.g. 64x48x32,256x256x256,1024x1024 (obs 33 / act 8, batch 256); layered ones run fsrl_bc_update_layered")
    ap.add_argument("--solo-window", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bc.py needs a GPU"
    if a.solo_window:
        return solo_window()
    if a.ks:
        doc = {"tool": "tools/bench_bc.py --ks", "unit": "us per member update, host clock around a window ending in a synchronise",
               "results": list(group_rows(a.ks))}
        if a.ab_tree:
            doc["solo_ab"] = solo_ab(a.ab_tree)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
        return
    results = []
    for hidden, Do, Da, B in ([(h, 33, 8, 256) for h in a.hidden] if a.hidden else SHAPES):
        rng = np.random.default_rng(0)
        (eng, hip), (_, ref) = hip_window(hidden, Do, Da, B, rng), torch_window(hidden, Do, Da, B, rng)
        hip(); ref()
        us = {"hip": [], "torch": []}
        n_hip = UPDATES if _layered(eng) else HIP_UPDATES
        for _ in range(ROUNDS):
            for name, fn, n in (("hip", hip, n_hip), ("torch", ref, UPDATES)):
                t0 = time.perf_counter(); fn(); us[name].append((time.perf_counter() - t0) * 1e6 / n)
        eng.close()
        row = {"hidden": list(hidden), "obs_dim": Do, "act_dim": Da, "batch": B, "updates_per_window": {"hip": n_hip, "torch": UPDATES}, "rounds": ROUNDS}
        for name, v in us.items():
            spread(row, name, v)
        results.append(row)
        print(json.dumps(row))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_bc.py", "unit": "us per update, host clock around a window ending in a synchronise", "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
