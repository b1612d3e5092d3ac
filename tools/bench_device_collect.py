#!/usr/bin/env python
"""env-steps/s of a collect loop (training mode: stochastic actions) on the linear env at obs 8 / act 2, episode length 300:

  (a) device     fsrl_collect_device: actor, noise, map_action, env step, store write and episode bookkeeping in one looping kernel
  (b) in-process FastCollector(device_actor=True) over SyntheticSafetyVectorEnv: the resident actor, one doorbell round trip per vector step
  (c) stepped    FastCollector(device_actor=True) over DeviceVectorEnv.step: the device env as an ordinary vector env (one launch per step)

for 20 and 64 envs at hidden (256, 256) and (64, 64).  Every round times `--calls` collects of env_num episodes per path, the paths
alternate inside a round; the result is the median over the rounds and their spread (max - min).  For (a) also the time per vector
step and per launch, at the default steps per launch and with the whole collect in one launch.

    python tools/bench_device_collect.py --rounds 3 --out profiles/device_collect.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fsrl_amd.data import DeviceCollector, FastCollector, HipVectorReplayBuffer  # noqa: E402
from fsrl_amd.engine import Engine, EngineConfig  # noqa: E402
from fsrl_amd.env import Box, DeviceLinear, SyntheticSafetyVectorEnv  # noqa: E402

EPISODE_LEN = 300


class Pol:
    """what the collectors read off a policy: training mode, clip, no scaling (the agents' defaults)"""
    traj_buffer = None
    training, _deterministic_eval = True, True
    action_bound_method, action_scaling = "clip", False

    def __init__(self, eng):
        self.engine = eng
        self.action_space = Box(-1.0, 1.0, (eng.cfg.act_dim, ))


def setup(path, hidden, n):
    eng = Engine(EngineConfig(obs_dim=8, act_dim=2, hidden=hidden, env_num=n, buffer_size=n * 2 * EPISODE_LEN), device=0)
    eng.set_params((0.1 * np.random.default_rng(0).standard_normal(eng.n_params)).astype(np.float32))
    host = SyntheticSafetyVectorEnv(env_num=n, obs_dim=8, act_dim=2, episode_len=EPISODE_LEN, seed=1)
    pol, buf = Pol(eng), HipVectorReplayBuffer(eng, n * 2 * EPISODE_LEN, n)
    if path == "in_process":
        return eng, None, FastCollector(pol, host, buf, device_actor=True)
    env = DeviceLinear(eng, like=host, seed=1)
    return eng, env, (DeviceCollector(pol, env, buf) if path == "device" else FastCollector(pol, env, buf, device_actor=True))


def timed(col, n, calls):
    col.reset_buffer()
    col.collect(n_episode=n)                          # warm: code objects, the resident kernel, the staging arrays
    col.reset_buffer()
    rows, t0 = 0, time.perf_counter()
    for _ in range(calls):
        rows += col.collect(n_episode=n)["n/st"]
        col.reset_buffer()
    return rows, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--envs", default="20,64")
    ap.add_argument("--hidden", default="256,64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    paths = ("device", "in_process", "stepped")
    result = dict(metric="env-steps/s of a collect loop, training mode, linear env obs 8 / act 2, episode length 300", rounds=a.rounds,
                  calls=a.calls, configs=[])
    for hidden in (int(h) for h in a.hidden.split(",")):
        for n in (int(e) for e in a.envs.split(",")):
            objs = {p: setup(p, hidden, n) for p in paths}
            rates = {p: [] for p in paths}
            for _ in range(a.rounds):
                for p in paths:
                    rows, dt = timed(objs[p][2], n, a.calls)
                    rates[p].append(rows / dt)
            cfg = dict(hidden=[hidden, hidden], env_num=n)
            for p in paths:
                cfg[p] = dict(median=float(np.median(rates[p])), spread=float(np.max(rates[p]) - np.min(rates[p])), rounds=[float(r) for r in rates[p]])
            # (a) per vector step and per launch: the default steps per launch, and the whole collect in one launch
            eng, env, col = objs["device"]
            for name, steps in (("default", 0), ("one_launch", EPISODE_LEN)):
                col.max_steps_per_launch = steps
                per_step, per_launch, launches = [], [], 0
                for _ in range(a.rounds):
                    rows, dt = timed(col, n, a.calls)
                    launches = col.last_launches
                    per_step.append(dt / a.calls / EPISODE_LEN * 1e6)
                    per_launch.append(dt / a.calls / launches * 1e6)
                cfg["device_" + name] = dict(launches_per_collect=launches, us_per_vector_step=float(np.median(per_step)),
                                             us_per_launch=float(np.median(per_launch)),
                                             us_per_vector_step_spread=float(np.max(per_step) - np.min(per_step)))
            col.max_steps_per_launch = 0
            result["configs"].append(cfg)
            print(json.dumps(cfg), flush=True)
            for eng, env, col in objs.values():
                if env is not None:
                    env.close()
                eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(device_collect=[(c["hidden"][0], c["env_num"], round(c["device"]["median"]), round(c["in_process"]["median"]),
                                           round(c["stepped"]["median"])) for c in result["configs"]])))


if __name__ == "__main__":
    main()
