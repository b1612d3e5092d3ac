"""The CPU preconditions of tests/test_gpu_devcollect_layered.py, in the style of tests/test_devcollect_shapes_model.py.  No GPU.

Every row-by-row case of tests/devcollect_layered_cases.py runs here as a closed loop of the float32 model with the oracles' CPU
actors over the layered hidden_sizes (devenv_replay_model.cpu_actor / cpu_onpolicy_actor take any depth):
  * the share of rows whose cost / terminated decision lies inside the discontinuity band is at most dm.BAND_CAP (2 %) -- a
    condition on the case (its seed, its env_num, its widths), under which the GPU test may compare discontinuous outputs at all;
  * costs occur, and terminations on the point-circle env: the decisions compared are not all one value.
And the cases keep the caps their issue set: at most 64 envs and 70 episodes, episodes cut at 7 steps."""
import functools

import numpy as np
import pytest

import devcollect_layered_cases as lc
import devenv_model as dm
import devenv_replay_model as rm
from fsrl_amd.engine import collect_device_layered, evaluate_device_layered  # noqa: F401  the calls these cases are collected through

F32, F64 = np.float32, np.float64
IDS = [lc.case_id(c) for c in lc.ALL_ROW_CASES]


@functools.lru_cache(maxsize=None)
def closed_loop(i, deterministic):
    agent, kind, n, n_ep, _, opts = case = lc.ALL_ROW_CASES[i]
    Do, Da = rm.SHAPES[kind]
    if kind == "pc":
        env = dm.ModelEnv(dm.POINT_CIRCLE, n, 7, rm.ENV_SEED, (rm.PC["radius"], rm.PC["x_lim"], rm.PC["dt"]), Do, Da, dtype=F32)
    else:
        host = rm.linear_host(kind, n)
        env = dm.ModelEnv(dm.LINEAR, n, 7, rm.ENV_SEED, (0.7, ), Do, Da, host.A, host.B, dtype=F32)
    actor = rm.case_actor(case)
    steps = []
    step = env.step
    env.step = lambda act, ids=None: steps.append(step(act, ids)) or steps[-1]

    def policy(obs, ids):
        m, sigma = actor(obs)
        eps32 = env.action_noise(ids, F32)
        if agent == "onpolicy" and not deterministic:       # the device's arithmetic: mu + sigma * eps, each operation rounded
            act = (m + sigma * eps32).astype(F32)
        else:
            act = rm.action(rm.formula(agent), m, sigma, eps32, deterministic, F32)
        return dm.map_action(act, 1)
    env.reset()
    rows, episodes, n_steps = dm.collect(env, n_ep, policy)
    assert episodes >= n_ep and len(steps) == n_steps and sum(len(s["rew"]) for s in steps) == len(rows)
    return dict(n_rows=len(rows), near=np.concatenate([dm.band_share(s)[1] for s in steps]), cost=sum(s["cost"].sum() for s in steps),
                terminated=sum(s["terminated"].sum() for s in steps))


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("i", range(len(lc.ALL_ROW_CASES)), ids=IDS)
def test_closed_loop_rows_stay_out_of_the_discontinuity_band(i, deterministic):
    kind = lc.ALL_ROW_CASES[i][1]
    r = closed_loop(i, deterministic)
    print(f"{IDS[i]} deterministic={deterministic}: {r['n_rows']} rows, cost rows {r['cost']:.0f}, terminations {r['terminated']}, "
          f"within the band {r['near'].mean():.4f}")
    assert r["near"].mean() <= dm.BAND_CAP == 0.02
    assert r["cost"] > 0
    if kind == "pc":
        assert r["terminated"] > 0


def test_cases_keep_the_caps_and_reach_the_kernel_edges():
    assert all(1 <= n <= lc.MAX_ENVS and 1 <= ep <= lc.MAX_EPISODES for n, ep in lc.all_sizes())
    envs = {n for n, _ in lc.all_sizes()}
    assert {1, 5, 16, 17, 64} <= envs                       # one row, part of a tile, a full tile, a tile and a row, four tiles
    widths = [hs for _, hs, _, _, _, _ in lc.TWIN_SHAPES]
    assert any(len(hs) == 1 for hs in widths) and any(len(hs) == 8 for hs in widths)
    assert any(w % 4 for hs in widths for w in hs)          # weight rows that are not 16-byte aligned
    assert any(w > 64 for hs in widths for w in hs)         # more than one 64-wide chunk of k, more than four column tiles
    assert any(forced and len(hs) == 2 and max(hs) <= 256 for _, hs, forced, _, _, _ in lc.TWIN_SHAPES)
    assert {c[0] for c in lc.ALL_ROW_CASES} == {"onpolicy", "sacl", "cvpo", "ddpgl"}
    assert any(rm.SHAPES[c[1]][1] == 8 for c in lc.ROW_CASES if c[0] == "sacl")          # SAC-Lag's 16 head columns
    assert any(rm.SHAPES[c[1]][1] == 16 for c in lc.ROW_CASES if c[0] == "ddpgl")
