"""Case table of the two-launch clipped PPO-Lagrangian step (ppo_wgrad_kernel<H, false, true, true>), its data and its oracle runs.
No GPU import here: tests/test_clip_fuse_problems_host.py proves on the oracle alone that every case reaches the branch it names,
tests/test_gpu_ppo_clip_fuse_shapes.py runs the cases on the device.

The weight-gradient kernel holds back up to five gradient elements per thread (ClipPend): slot k of the dW1 role is the element of
observation columns 16 k .. 16 k + 15, so slots 1, 2, 3 exist only above 16, 32, 48 columns and the host refuses the route above 64.
Every dimension of a shape case is the smallest that still reaches its branch.  The rows of a case come from ragged environments
(different lengths, one of them short), in the store's env-major order, with truncations, one termination per longer environment and an
unfinished tail per environment.  Every case runs max_grad_norm 0.5, lagrangian 0.5, rescaling 1 / 1.5 and parameters 0.1 * randn
unless its row says otherwise."""
import functools
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import numpy as np

LAGRANGIAN, RESCALING = 0.5, 1.0 / 1.5


@dataclass(frozen=True)
class Case:
    id: str
    shape: str                       # the shape case whose data it runs on
    obs: int
    act: int
    critics: int
    H: int
    rows: Tuple[int, ...]            # rows per environment
    batch: int
    minibatches: Tuple[int, ...]     # what split_chunks makes of sum(rows) / batch, per pass
    passes: int = 2
    max_grad_norm: float = 0.5
    opts: Tuple[Tuple[str, object], ...] = ()      # EngineConfig fields away from their defaults
    refused: bool = False            # the host must keep three launches (clip_fuse_update_ok)
    own_actions: bool = False        # actions drawn from the initial policy: the KL estimate grows with the passes
    target_kl: Optional[float] = None
    seed: int = 0                    # of the data, chosen where the host test's conditions on the norms need it
    stop_pass: int = -1              # with target_kl: the pass whose mean KL first exceeds 1.5 * target_kl
    reaches: str = ""

    @property
    def n(self):
        return sum(self.rows)

    @property
    def fused_steps(self):
        """two-launch steps of one update: minibatches of at most 512 padded rows x passes run (none where the route is refused)"""
        if self.refused:
            return 0
        per_pass = sum(1 for m in self.minibatches if -(-m // 16) * 16 <= 512)
        return per_pass * (self.stop_pass + 1 if self.target_kl else self.passes)

    @property
    def steps(self):
        return len(self.minibatches) * (self.stop_pass + 1 if self.target_kl else self.passes)


def _shape(id, obs, act, critics, H, rows, batch, minibatches, reaches, **kw):
    return Case(id, id, obs, act, critics, H, tuple(rows), batch, tuple(minibatches), reaches=reaches, **kw)


SHAPES = {c.id: c for c in (
    _shape("o17", 17, 1, 2, 128, (300, 257, 43), 256, (256, 344), "slot 1 with one column; H 128; the narrowest head"),
    _shape("o33a16", 33, 16, 1, 256, (400, 509, 100), 504, (504, 505),
           "slot 2; sigma on threads 16-31; two networks; both steps padded to 512 rows (the upper edge of clip_fuse_step_ok)"),
    _shape("o49tiny", 49, 6, 2, 64, (20, 1, 24), 8, (8, 8, 8, 8, 13), "slot 3; one tile, KS = 4, twelve idle waves; 4-row tile plan"),
    _shape("o64mix", 64, 3, 2, 128, (500, 400, 125), 512, (512, 513), "slot 3 full; 513 rows take the split-K route inside the update"),
    _shape("o16", 16, 2, 1, 64, (4, 1, 2), 1000, (7,), "slot 0 full, slot 1 empty; one minibatch of seven rows", seed=2),
    _shape("o32a16", 32, 16, 2, 128, (250, 250, 100), 256, (256, 344), "slot 1 full, slot 2 empty"),
    _shape("o48", 48, 1, 1, 256, (30, 15), 8, (8, 8, 8, 8, 13), "slot 2 full, slot 3 empty; 163-block grid"),
    _shape("o65", 65, 2, 2, 64, (300, 257, 43), 256, (256, 344), "refused: above CLIP_FUSE_MAX_OBS", refused=True),
)}

# measured with the float64 oracle: o49tiny's ten sequential pre-clip norms under this threshold lie on both sides of it, none within 2 %
# (tests/test_clip_fuse_problems_host.py holds that)
STRADDLE_NORM = 2.45

CLIP_BRANCH = {c.id: c for c in (
    replace(SHAPES["o49tiny"], id="o49tiny-loose", max_grad_norm=100.0, reaches="coefficient exactly 1 in every step"),
    replace(SHAPES["o17"], id="o17-loose", max_grad_norm=100.0, reaches="coefficient exactly 1 in every step"),
    replace(SHAPES["o49tiny"], id="o49tiny-straddle", max_grad_norm=STRADDLE_NORM, reaches="steps that clip and steps that do not in one update"),
)}

_OPTION_SETS = {
    "dual": (("dual_clip", 1.5), ("norm_adv", False), ("lr", 3e-3)),
    "nolag": (("use_lagrangian", False), ("unbounded", True), ("beta1", 0.8), ("beta2", 0.99)),
    "wide": (("max_action", 1.5), ("dual_clip", 1.5), ("beta1", 0.8), ("beta2", 0.99), ("lr", 3e-3)),
}
OPTIONS = {f"{s}-{name}": replace(SHAPES[s], id=f"{s}-{name}", opts=opts, reaches="options " + ", ".join(k for k, _ in opts))
           for s in ("o33a16", "o17") for name, opts in _OPTION_SETS.items()}

# these two options turn the route off by design (a replay would not reproduce the update): refused like o65
REFUSED = {c.id: c for c in (
    SHAPES["o65"],
    replace(SHAPES["o17"], id="o17-rewnorm", opts=(("rew_norm", True),), refused=True, reaches="refused: reward normalisation"),
    replace(SHAPES["o17"], id="o17-recompute", opts=(("recompute_adv", True),), refused=True, reaches="refused: recomputed advantages"),
)}

# The logged KL is mean(logp_old - logp): on actions the policy did not draw it drifts below zero, so these cases draw their actions from
# the initial policy and learn at 3e-3.  target_kl puts 1.5 * target_kl between the mean KL of pass stop_pass and the largest before
# it, at least 20 % from both (held by the host test on the fp32 and the float64 oracle); one pass more is asked for than the stop allows.
KL = {c.id: c for c in (
    replace(SHAPES["o17"], id="o17-kl", opts=(("lr", 3e-3),), own_actions=True, target_kl=0.005 / 1.5, stop_pass=1, passes=3,
            reaches="KL stop after the second pass"),
    replace(SHAPES["o33a16"], id="o33a16-kl", opts=(("lr", 3e-3),), own_actions=True, target_kl=0.33, stop_pass=1, passes=3,
            reaches="KL stop after the second pass"),
)}

FUSED = {**{k: v for k, v in SHAPES.items() if not v.refused}, **CLIP_BRANCH, **OPTIONS}
CASES = {**FUSED, **REFUSED, **KL}

_TO_ORACLE = dict(dual_clip="dual_clip", norm_adv="advantage_normalization", use_lagrangian="use_lagrangian", unbounded="unbounded",
                  max_action="max_action", lr="lr", rew_norm="reward_normalization", recompute_adv="recompute_advantage")


def lagrangians(case):
    return np.full(case.critics - 1, LAGRANGIAN)


def engine_kwargs(case, **over):
    """EngineConfig fields of a case"""
    kw = dict(env_num=len(case.rows), buffer_size=len(case.rows) * 1024, obs_dim=case.obs, act_dim=case.act, hidden=case.H,
              n_critics=case.critics, max_grad_norm=case.max_grad_norm, target_kl=case.target_kl)
    kw.update(dict(case.opts))
    kw.update(over)
    return kw


def oracle_config(case, **over):
    from oracle.ppo_lag import PPOLagConfig
    o = dict(case.opts)
    kw = dict(obs_dim=case.obs, act_dim=case.act, hidden=(case.H, case.H), n_critics=case.critics, max_grad_norm=case.max_grad_norm,
              target_kl=case.target_kl if case.target_kl else 1e9, betas=(o.pop("beta1", 0.9), o.pop("beta2", 0.999)))
    kw.update({_TO_ORACLE[k]: v for k, v in o.items()})
    kw.update(over)
    return PPOLagConfig(**kw)


@functools.lru_cache(maxsize=None)
def _problem(shape, own_actions):
    from oracle.ppo_lag import OnPolicyData
    c = SHAPES[shape]
    rng = np.random.default_rng(1000 * c.obs + c.H + c.n + 100000 * c.seed)
    ep = max(2, max(c.rows) // 3)                     # two truncations in the longest environment
    env = []
    for T in c.rows:
        obs = rng.standard_normal((T + 1, c.obs)).astype(np.float32)
        act = (0.3 * rng.standard_normal((T, c.act))).astype(np.float32)
        rew = rng.normal(0.5, 0.5, T); cost = (rng.random(T) < 0.2).astype(np.float64)
        trunc = np.zeros(T, bool); trunc[ep - 1::ep] = True
        term = np.zeros(T, bool)
        if T > 3:
            term[T // 2] = True
        env.append(dict(obs=obs[:-1], act=act, rew=rew, cost=cost, term=term, trunc=trunc, obs_next=obs[1:]))
    theta_rng = np.random.default_rng(3)
    n_params = _n_params(c)
    theta = (0.1 * theta_rng.standard_normal(n_params)).astype(np.float32)
    if own_actions:
        import torch
        from oracle.ppo_lag import PPOLagOracle
        o = PPOLagOracle(oracle_config(c), dtype=torch.float64)
        o.set_params(theta)
        arng = np.random.default_rng(5)
        for e in env:
            with torch.no_grad():
                d = o.actor_dist(torch.as_tensor(e["obs"], dtype=torch.float64)).base_dist
            e["act"] = (d.loc.numpy() + d.scale.numpy() * arng.standard_normal(e["act"].shape)).astype(np.float32)
    cat = {k: np.concatenate([e[k] for e in env]) for k in env[0]}
    end = (cat["term"] | cat["trunc"]).copy()
    end[np.cumsum(c.rows) - 1] = True                  # unfinished tails
    data = OnPolicyData(obs=cat["obs"], act=cat["act"], rew=cat["rew"], cost=cat["cost"], terminated=cat["term"],
                        truncated=cat["trunc"], obs_next=cat["obs_next"], end_flag=end)
    perms = [rng.permutation(c.n) for _ in range(8)]
    return dict(env=env, data=data, theta=theta, perms=perms)


def _n_params(c):
    from oracle import layout
    return sum(layout.spec_size(s) for s in layout.onpolicy_specs(c.obs, c.act, (c.H, c.H), c.critics))


def problem(case):
    """-> dict(env: per-environment columns, data: OnPolicyData in store order, theta, perms); shared: callers leave it unchanged"""
    return _problem(case.shape, case.own_actions)


def fill(eng, case):
    """the case's parameters and rows into an engine: lock-step pushes, environments drop out as they run dry"""
    p = problem(case)
    eng.set_params(p["theta"])
    for t in range(max(case.rows)):
        ids = [e for e in range(len(case.rows)) if t < case.rows[e]]
        eng.push(ids, *[np.stack([p["env"][e][k][t] for e in ids]) for k in ("obs", "act", "rew", "cost", "term", "trunc", "obs_next")])


@functools.lru_cache(maxsize=None)
def _oracle_run(case_id, f64, passes, no_stop, max_grad_norm):
    import torch
    from oracle.ppo_lag import PPOLagOracle
    torch.set_num_threads(4)
    case = CASES[case_id]
    over = {}
    if no_stop:
        over["target_kl"] = 1e9
    if max_grad_norm is not None:
        over["max_grad_norm"] = max_grad_norm
    p = problem(case)
    o = PPOLagOracle(oracle_config(case, **over), dtype=torch.float64 if f64 else torch.float32)
    o.set_params(p["theta"])
    norms = []
    _, stats, stopped = o.update(p["data"], lagrangians(case), RESCALING, case.batch, passes, perms=p["perms"][:passes], grad_norms=norms)
    out = dict(stats=np.asarray(stats, np.float64), params=o.get_params(), norms=np.asarray(norms, np.float64), stopped=stopped)
    return out


def oracle_run(case, f64, passes=None, no_stop=False, max_grad_norm=None):
    """the fp32 (reference-equivalent) or float64 oracle on a case -> dict(stats [steps, 11], params, norms [steps]: the pre-clip
    gradient norm of every step, stopped); computed once, shared: callers leave it unchanged"""
    return _oracle_run(case.id, bool(f64), case.passes if passes is None else passes, bool(no_stop), max_grad_norm)


def pass_kl(stats, n_minibatches):
    """mean logged KL of every pass"""
    return np.asarray(stats)[:, 5].reshape(-1, n_minibatches).mean(axis=1)
