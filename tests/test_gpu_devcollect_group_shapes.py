"""Grouped device collects (fsrl_collect_device_group) at the widths and kernels that tests/test_gpu_devcollect_group.py launches at 64
wide only: the 128- and 256-wide LINEAR-env instantiations of collect_device_group_kernel for the on-policy head, the grouped replay-head
kernels at 128 and 256 wide, and members that differ in everything their own row of the member table carries.

The oracle is that file's: fsrl_collect_device on an ungrouped twin of every member, bit for bit -- rows, sizes, books, env state,
statistics, store_version, and the sum tree of a prioritised member.  The solo call at the same shapes is held to the float64 model
by tests/test_gpu_devcollect_shapes.py; that a neighbour's max_action or exploration_sigma would miss the true action by 100 bounds
is asserted without a GPU in tests/test_devcollect_shapes_model.py."""
import numpy as np
import pytest

import devenv_replay_model as rm
import test_gpu_devcollect_group as gp
import test_gpu_devcollect_shapes as sh

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.mark.parametrize("H", [128, 256])
def test_onpolicy_members_of_an_update_group_equal_their_twins(H):
    """lin8 with env_num 1 / 17 / 64, 8 vector steps per launch, a second round after set_params on every member"""
    gp.onpolicy_members_equal_their_twins(H)


@pytest.mark.parametrize("agent,kind,H", [("sacl", "lin33", 256), ("ddpgl", "lin64w", 256), ("cvpo", "lin8", 256), ("sacl", "lin33", 128),
                                          ("ddpgl", "lin64w", 128)])
def test_replay_members_equal_their_twins(agent, kind, H):
    """SAC-Lag (prioritised replay on) at SAC-Lag's full 16-column head row, DDPG-Lag at its widest head over obs 64, CVPO"""
    gp.replay_members_equal_their_twins(agent, kind, H)


@pytest.mark.parametrize("agent", sorted(rm.GROUP_DIFF_CASES))
def test_members_that_differ_in_their_own_arguments_equal_their_twins(agent):
    """three ungrouped members of one launch with max_action 1.0 / 1.5 / 0.5 (DDPG-Lag: exploration_sigma 0.1 / 0.3 / 0.05 too),
    their own bounds, env_num, n_episode and env seed; a member that read another member's row would not equal its twin"""
    cases = rm.GROUP_DIFF_CASES[agent]
    n_eps = [c[3] for c in cases]
    lows = np.array([[-2.0, -0.5], [-1.0, -1.5], [-0.25, -3.0]], F32)
    highs = np.array([[0.5, 1.0], [2.0, 0.75], [1.5, 0.5]], F32)
    mem = [sh.build(c, seed=5 + i, rows_per_env=9) for i, c in enumerate(cases)]
    twin = [sh.build(c, seed=5 + i, rows_per_env=9) for i, c in enumerate(cases)]
    for _, v in mem + twin:
        v.reset()
    for rnd, (cut, det) in enumerate(((5, False), (0, False), (0, True))):
        res = gp.group_collect([e for e, _ in mem], [v for _, v in mem], n_eps, deterministic=det, bound_method=1, lows=lows, highs=highs,
                               max_steps_per_launch=cut)
        for i, (e, v) in enumerate(twin):
            solo = e.collect_device(v._h, n_eps[i], deterministic=det, bound_method=1, low=lows[i], high=highs[i], max_steps_per_launch=cut)
            gp.assert_same_stats(res[i], solo, f"{agent} round {rnd} member {i}")
            gp.assert_same_snapshot(gp.snapshot(*mem[i]), gp.snapshot(*twin[i]), f"{agent} round {rnd} member {i}")
        if rnd == 0:
            assert res[0]["launches"] > 1
        if rnd == 1 and agent != "ddpgl":                   # max_action 1.5 in training mode: stored actions beyond +-1 met the clip
            assert np.abs(gp.on.store_rows(mem[1][0])[1]["act"]).max() > 1.0
    for i in range(3):
        assert mem[i][0].store_sizes().max() == 9           # the sub-buffers wrapped
        assert all(np.array_equal(x, y) for x, y in zip(gp.books(mem[i][0]), gp.books(twin[i][0]))), f"member {i}: books"
    gp.close(*[v for _, v in mem + twin]); gp.close(*[e for e, _ in mem + twin])
