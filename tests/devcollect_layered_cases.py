"""The cases of tests/test_gpu_devcollect_layered.py, whose CPU preconditions tests/test_devcollect_layered_model.py asserts.  TEST
INFRASTRUCTURE ONLY.  No GPU is touched here.

Shapes are the smallest at which lay_collect_kernel (fsrl_amd/csrc/kernels_devcollect_layered.hpp) can go wrong: one and several
row tiles (1 / 5 / 16 / 17 / 64 envs), one and several column tiles, K below / at / above one 16-wide sub-chunk and one 64-wide
chunk (6, 8, 16, 18, 30, 32, 33, 50, 64, 512), weight rows that are and are not 16-byte aligned (K = 33, 50, 30, 18 are not), one
and eight hidden layers, and a two-layer network forced through the layered kernels.  Episodes are cut at 7 steps."""
import devenv_replay_model as rm

# ---- deterministic twins: (id, hidden_sizes, force_layered, env kind, env_num, episodes of the two collects)
TWIN_SHAPES = [
    ("h32x32x32-pc-n5", (32, 32, 32), False, "pc", 5, (3, 12)),
    ("h50x30x18-lin33-n17", (50, 30, 18), False, "lin33", 17, (20, 9)),       # unaligned rows; K = 33, 50, 30; a second tile of one row
    ("h64-lin8-n1", (64, ), False, "lin8", 1, (2, 1)),
    ("h16x8-lin8-n16", (16, ) * 8, False, "lin8", 16, (16, 30)),
    ("h512x512-lin8-n64", (512, 512), False, "lin8", 64, (70, 64)),           # four row tiles, eight 64-chunks
    ("h64x64forced-pc-n5", (64, 64), True, "pc", 5, (5, 5)),
]
# (id, action_bound_method, (low, high) or None): the default, bounds with a bound method, bounds without one
TWIN_BOUNDS = [("clip", "clip", None), ("clip-bounds", "clip", (-2.0, 0.5)), ("nomethod-bounds", "", (-0.5, 1.5))]
# the on-policy head's two options, at the widths of the second shape's env: (id, EngineConfig options)
TWIN_HEADS = [("unbounded", dict(unbounded=True)), ("max_action1.5", dict(max_action=1.5))]
TWIN_HEAD_SHAPE = ("h32x32x32-lin8-n17", (32, 32, 32), False, "lin8", 17, (20, 9))

# ---- training mode, row by row: cases in the form of devenv_replay_model.SHAPE_CASES
# (agent or "onpolicy", env kind, env_num, n_episode, unused, {"hidden_sizes": ...}); the env seed is rm.ENV_SEED
ROW_CASES = [
    ("onpolicy", "lin33", 5, 12, 0, {"hidden_sizes": (50, 30, 18)}),
    ("onpolicy", "pc", 17, 25, 0, {"hidden_sizes": (32, 32, 32)}),
    ("sacl", "lin33", 5, 12, 0, {"hidden_sizes": (32, 32, 32)}),             # act 8: the full 16-column head row
    ("cvpo", "lin8", 64, 70, 0, {"hidden_sizes": (48, 24, 40)}),
    ("ddpgl", "lin20", 5, 12, 0, {"hidden_sizes": (32, 32, 32)}),            # act 16
]
# the prioritised case: SAC-Lag, its rows against the model AND its tree against the stepped twin's
PER_CASE = ("sacl", "pc", 5, 8, 0, {"hidden_sizes": (32, 32, 32)})
ALL_ROW_CASES = ROW_CASES + [PER_CASE]

# ---- groups: three members with different env_num, n_episode and env seeds, one shape
GROUP_HIDDEN = (32, 32, 32)
GROUP_MEMBERS = [(5, 12, 3), (17, 25, 4), (3, 8, 9)]        # (env_num, n_episode, env seed)

MAX_ENVS, MAX_EPISODES = 64, 70


def case_id(case):
    return rm.case_id(case).replace(" ", "")


def all_sizes():
    """(env_num, n_episode) of every case, for the caps of the issue"""
    out = [(n, ep) for _, _, _, _, n, eps in TWIN_SHAPES + [TWIN_HEAD_SHAPE] for ep in eps]
    out += [(c[2], c[3]) for c in ALL_ROW_CASES] + [(n, ep) for n, ep, _ in GROUP_MEMBERS]
    return out
