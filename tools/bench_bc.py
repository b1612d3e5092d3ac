"""Microseconds per behaviour-cloning update (fsrl_bc_update) next to the same regression in stock torch (torch.nn + torch.optim.Adam)
on the same GPU.  Shapes: 256 x 256, obs 33 / act 8, batch 256 and 1024; 64 x 64, obs 6 / act 2, batch 256.  Every window is UPDATES
(torch) or HIP_UPDATES (fsrl_bc_update: windows of a few hundred ms) updates and ends in a device synchronise; the HIP window includes
the host's draw of its batch x updates indices, torch draws on the device; the two paths alternate, ROUNDS rounds after a warm-up window of each; median and min - max.
    python tools/bench_bc.py [--out profiles/bc_update.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fsrl_amd.engine import Engine, EngineConfig

SHAPES = [((256, 256), 33, 8, 256), ((256, 256), 33, 8, 1024), ((64, 64), 6, 2, 256)]
ROWS, UPDATES, HIP_UPDATES, ROUNDS = 4096, 2000, 10000, 7


def hip_window(hidden, Do, Da, B, rng):
    eng = Engine(EngineConfig(obs_dim=Do, act_dim=Da, hidden_sizes=hidden, env_num=16, buffer_size=ROWS), device=0)
    eng.set_params((0.1 * rng.standard_normal(eng.n_params)).astype(np.float32))
    ids, z, f = np.arange(16), np.zeros(16), np.zeros(16, bool)
    for _ in range(ROWS // 16):
        o = rng.standard_normal((16, Do)).astype(np.float32)
        eng.push(ids, o, np.tanh(rng.standard_normal((16, Da))).astype(np.float32), z, z, f, f, o)
    return eng, lambda: eng.bc_update(B, HIP_UPDATES, loss="mse", seed=1)      # returns the losses: synchronises


def torch_window(hidden, Do, Da, B, rng):
    dev = torch.device("cuda:0")
    net = torch.nn.Sequential(torch.nn.Linear(Do, hidden[0]), torch.nn.ReLU(), torch.nn.Linear(hidden[0], hidden[1]), torch.nn.ReLU(),
                              torch.nn.Linear(hidden[1], Da), torch.nn.Tanh()).to(dev)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bc.py needs a GPU"
    results = []
    for hidden, Do, Da, B in SHAPES:
        rng = np.random.default_rng(0)
        (eng, hip), (_, ref) = hip_window(hidden, Do, Da, B, rng), torch_window(hidden, Do, Da, B, rng)
        hip(); ref()
        us = {"hip": [], "torch": []}
        for _ in range(ROUNDS):
            for name, fn, n in (("hip", hip, HIP_UPDATES), ("torch", ref, UPDATES)):
                t0 = time.perf_counter(); fn(); us[name].append((time.perf_counter() - t0) * 1e6 / n)
        eng.close()
        row = {"hidden": list(hidden), "obs_dim": Do, "act_dim": Da, "batch": B, "updates_per_window": {"hip": HIP_UPDATES, "torch": UPDATES}, "rounds": ROUNDS}
        for name, v in us.items():
            row[name + "_us_median"], row[name + "_us_min"], row[name + "_us_max"] = float(np.median(v)), min(v), max(v)
        results.append(row)
        print(json.dumps(row))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_bc.py", "unit": "us per update, host clock around a window ending in a synchronise", "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
