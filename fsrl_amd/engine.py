"""numpy-facing wrapper of one libfsrl_hip context (one per GPU / per agent).

This is plumbing: every method forwards to one C-ABI entry point of include/fsrl_hip.h.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib

_f32p, _f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
_u8p, _i32p, _i64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def _ptr(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def mem_live():
    """Device and pinned blocks / bytes the library holds in this process right now (fsrl_mem_live)."""
    v = [C.c_int64(0) for _ in range(4)]
    _lib.check(_lib.load().fsrl_mem_live(*[C.byref(x) for x in v]))
    return dict(zip(("dev_blocks", "dev_bytes", "pinned_blocks", "pinned_bytes"), (x.value for x in v)))


@dataclass
class EngineConfig:
    """Mirror of struct fsrl_config; defaults = PPOLagAgent defaults (ppo_lag_agent.py:82-116)."""
    obs_dim: int = 8
    act_dim: int = 2
    hidden: int = 128                 # two hidden layers of this width ...
    hidden_sizes: Optional[Sequence[int]] = None   # ... or the agents' hidden_sizes (wins over `hidden`): two layers of at most 256
                                                   # units run on the fused kernels; any other tuple (1 .. 8 layers, any width)
                                                   # makes a layered context (include/fsrl_hip.h fsrl_config.n_hidden)
    force_layered: bool = False       # tests: a two-layer network through the layered kernels too
    n_critics: int = 2
    env_num: int = 20
    buffer_size: int = 100000
    max_action: float = 1.0
    gamma: float = 0.99
    gae_lambda: float = 0.95
    eps_clip: float = 0.2
    dual_clip: Optional[float] = None
    vf_coef: float = 0.25
    max_grad_norm: Optional[float] = None
    target_kl: float = 0.02
    norm_adv: bool = True
    use_lagrangian: bool = True
    lr: float = 5e-4
    beta1: float = 0.9
    beta2: float = 0.999
    adam_eps: float = 1e-8
    recompute_adv: bool = False
    unbounded: bool = False           # on-policy actor head without max_action * tanh
    rew_norm: bool = False            # reward_normalization (base_policy.py:430-444)
    value_clip: bool = False          # PPO clipped value loss (needs rew_norm)
    algo: int = _lib.ALGO_PPO_LAG

    def to_c(self):
        c = _lib.Config()
        c.algo, c.obs_dim, c.act_dim, c.hidden = self.algo, self.obs_dim, self.act_dim, self.hidden
        if self.hidden_sizes is not None:
            hs = [int(h) for h in self.hidden_sizes]
            if not 1 <= len(hs) <= 8:
                raise ValueError(f"the HIP path runs MLPs with 1 to 8 hidden layers, got hidden_sizes={tuple(hs)}")
            c.hidden, c.n_hidden = 0, len(hs)
            for i, h in enumerate(hs):
                c.hidden_sizes[i] = h
            c.force_layered = int(self.force_layered)
        c.n_critics, c.env_num, c.buffer_size = self.n_critics, self.env_num, self.buffer_size
        c.max_action, c.gamma, c.gae_lambda = self.max_action, self.gamma, self.gae_lambda
        c.eps_clip, c.dual_clip = self.eps_clip, (self.dual_clip or 0.0)
        c.vf_coef, c.max_grad_norm = self.vf_coef, (self.max_grad_norm or 0.0)
        tk = self.target_kl
        c.target_kl = 0.0 if (tk is None or not np.isfinite(tk) or tk >= 1e8) else tk
        c.norm_adv, c.use_lagrangian = int(self.norm_adv), int(self.use_lagrangian)
        c.lr, c.beta1, c.beta2, c.adam_eps = self.lr, self.beta1, self.beta2, self.adam_eps
        c.recompute_adv = int(self.recompute_adv)
        c.unbounded, c.rew_norm, c.value_clip = int(self.unbounded), int(self.rew_norm), int(self.value_clip)
        return c


class Engine:
    def __init__(self, cfg: EngineConfig, device: int = 0):
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = int(device)
        self._ctx = C.c_void_p()
        ccfg = cfg.to_c()
        _lib.check(self.lib.fsrl_ctx_create(int(device), C.byref(ccfg), C.byref(self._ctx)))
        self.n_params = int(self.lib.fsrl_param_count(self._ctx))
        self._act_stage = None
        self._collect_stage = None
        self._run_stage = None      # cached staging arrays + ctypes pointers of the collector's hot calls
        self._push_stage = None

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self.lib.fsrl_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _lib.check(self.lib.fsrl_sync(self._ctx))

    # ---------------------------------------------------------------- parameters
    def set_params(self, flat):
        flat = np.ascontiguousarray(flat, np.float32)
        _lib.check(self.lib.fsrl_params_set(self._ctx, _ptr(flat, _f32p), flat.size))

    def get_params(self):
        out = np.empty(self.n_params, np.float32)
        _lib.check(self.lib.fsrl_params_get(self._ctx, _ptr(out, _f32p), out.size))
        return out

    def get_grads(self):
        out = np.empty(self.n_params, np.float32)
        _lib.check(self.lib.fsrl_grads_get(self._ctx, _ptr(out, _f32p), out.size))
        return out

    def state_snapshot(self):
        """Checkpoint parameters + Adam state in HBM (device-to-device, asynchronous)."""
        _lib.check(self.lib.fsrl_state_snapshot(self._ctx))

    def state_restore(self):
        _lib.check(self.lib.fsrl_state_restore(self._ctx))

    def train_state_array(self, with_store: bool = True) -> np.ndarray:
        """train_state() as the uint8 array the library wrote into: no second copy of a store of hundreds of megabytes"""
        n = int(self.lib.fsrl_train_state_size(self._ctx, int(bool(with_store))))
        if n < 0:
            _lib.check(n)
        buf = np.empty(n, np.uint8)
        written = C.c_int64()
        _lib.check(self.lib.fsrl_train_state_export(self._ctx, int(bool(with_store)), buf.ctypes.data, n, C.byref(written)))
        return buf[:written.value]

    def train_state(self, with_store: bool = True) -> bytes:
        """The context's full training state as bytes (fsrl_train_state_export): parameters, optimiser state, random streams,
        running statistics and, with_store, the transition store.  A pure function of the state; env state is not in it."""
        return self.train_state_array(with_store).tobytes()

    def load_train_state(self, blob) -> None:
        """fsrl_train_state_import: everything about `blob` (bytes or a uint8 array) is checked before the first write, so a
        refused blob (AssertionError naming the reason) leaves the context as it was."""
        a = np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else np.ascontiguousarray(blob, np.uint8).reshape(-1)
        keep = a if a.size else np.zeros(8, np.uint8)         # an empty blob is refused by the validator, like any other
        _lib.check(self.lib.fsrl_train_state_import(self._ctx, keep.ctypes.data, a.size))

    def copy_train_state_from(self, other: "Engine", with_store: bool = True) -> None:
        """fsrl_train_state_copy: `other`'s training state into this context, device to device (same device, same shapes)."""
        _lib.check(self.lib.fsrl_train_state_copy(self._ctx, other._ctx, int(bool(with_store))))

    def optim_reset(self):
        _lib.check(self.lib.fsrl_optim_reset(self._ctx))

    def ret_rms_get(self) -> np.ndarray:
        """[n_critics, 3] running (mean, var, count) of the normalised returns (BasePolicy.ret_rms)."""
        out = np.zeros(3 * self.cfg.n_critics, np.float64)
        _lib.check(self.lib.fsrl_ret_rms_get(self._ctx, _ptr(out, _f64p), out.size))
        return out.reshape(-1, 3)

    def ret_rms_set(self, rms):
        v = np.ascontiguousarray(rms, np.float64).reshape(-1)
        _lib.check(self.lib.fsrl_ret_rms_set(self._ctx, _ptr(v, _f64p), v.size))

    def set_lr(self, group: int, lr: float):
        """Learning rate of one optimiser (fsrl_set_lr): what lr_scheduler.step() produced on the host."""
        _lib.check(self.lib.fsrl_set_lr(self._ctx, int(group), float(lr)))

    def get_lr(self, group: int = 0) -> float:
        return float(self.lib.fsrl_get_lr(self._ctx, int(group)))

    def ppo_abort(self):
        _lib.check(self.lib.fsrl_ppo_abort(self._ctx))

    # ---------------------------------------------------------------- store
    def push(self, env_ids, obs, act, rew, cost, terminated, truncated, obs_next):
        """VectorReplayBuffer.add for k rows -> (ptr, ep_rew, ep_len, ep_idx).  Called once per vector step:
        inputs are copied into cached staging arrays whose ctypes pointers are built once."""
        k = len(env_ids)
        st = self._push_stage
        if st is None or st["cap"] < k:
            cap, Do, Da = max(k, self.cfg.env_num), self.cfg.obs_dim, self.cfg.act_dim
            arr = dict(ids=np.empty(cap, np.int32), obs=np.empty((cap, Do), np.float32), act=np.empty((cap, Da), np.float32),
                       rew=np.empty(cap, np.float64), cost=np.empty(cap, np.float64), term=np.empty(cap, np.uint8),
                       trunc=np.empty(cap, np.uint8), nxt=np.empty((cap, Do), np.float32), ptr=np.empty(cap, np.int64),
                       er=np.empty(cap, np.float64), el=np.empty(cap, np.int32), ei=np.empty(cap, np.int64))
            types = dict(ids=_i32p, obs=_f32p, act=_f32p, rew=_f64p, cost=_f64p, term=_u8p, trunc=_u8p, nxt=_f32p, ptr=_i64p,
                         er=_f64p, el=_i32p, ei=_i64p)
            st = self._push_stage = dict(cap=cap, a=arr, p={n: _ptr(arr[n], types[n]) for n in arr})
        a, p = st["a"], st["p"]
        obs = np.asarray(obs, np.float32).reshape(k, -1); act = np.asarray(act, np.float32).reshape(k, -1)
        assert obs.shape[1] == self.cfg.obs_dim and act.shape[1] == self.cfg.act_dim
        a["ids"][:k] = env_ids; a["obs"][:k] = obs; a["act"][:k] = act; a["rew"][:k] = rew
        a["term"][:k] = terminated; a["trunc"][:k] = truncated
        a["nxt"][:k] = np.asarray(obs_next, np.float32).reshape(k, -1)
        if cost is not None:
            a["cost"][:k] = cost
        _lib.check(self.lib.fsrl_store_push(self._ctx, p["ids"], k, p["obs"], p["act"], p["rew"],
                                            p["cost"] if cost is not None else None, p["term"], p["trunc"], p["nxt"],
                                            p["ptr"], p["er"], p["el"], p["ei"]))
        return a["ptr"][:k].copy(), a["er"][:k].copy(), a["el"][:k].copy(), a["ei"][:k].copy()

    def reset_store(self, keep_statistics=False):
        _lib.check(self.lib.fsrl_store_reset(self._ctx, int(keep_statistics)))

    def __len__(self):
        return int(self.lib.fsrl_store_len(self._ctx))

    def store_read(self, indices):
        """buffer[indices] -> dict(obs, act, rew, cost, terminated, truncated, obs_next) on the host."""
        idx = np.ascontiguousarray(indices, np.int64).reshape(-1)
        n, Do, Da = idx.size, self.cfg.obs_dim, self.cfg.act_dim
        out = dict(obs=np.empty((n, Do), np.float32), act=np.empty((n, Da), np.float32), rew=np.empty(n, np.float64),
                   cost=np.empty(n, np.float64), terminated=np.empty(n, np.uint8), truncated=np.empty(n, np.uint8),
                   obs_next=np.empty((n, Do), np.float32))
        _lib.check(self.lib.fsrl_store_read(self._ctx, _ptr(idx, _i64p), n, _ptr(out["obs"], _f32p), _ptr(out["act"], _f32p),
                                            _ptr(out["rew"], _f64p), _ptr(out["cost"], _f64p), _ptr(out["terminated"], _u8p),
                                            _ptr(out["truncated"], _u8p), _ptr(out["obs_next"], _f32p)))
        out["terminated"] = out["terminated"].astype(bool); out["truncated"] = out["truncated"].astype(bool)
        return out

    def store_fill(self, archive: "TrajArchive", episode_ids=None, first_env: int = 0, bound_method: int = 0, low=None, high=None) -> int:
        """fsrl_store_fill: pour alive episodes of `archive` (episode_ids = None: all, in table order) into this engine's store, episode
        j into sub-buffer (first_env + j) % buffer_num, as if every row went through push() with map_action_inverse(actions) under
        (bound_method, low, high) -- one host-to-device copy of a job table and one launch.  Under tanh the action is clamped to
        +-(1 - 2**-24) before the inverse (the reference returns +-inf at +-1).  -> the rows the push loop would have pushed."""
        ids = None if episode_ids is None else np.ascontiguousarray(episode_ids, np.int32).reshape(-1)
        n = 0 if ids is None else ids.size
        if ids is not None and n == 0:
            ids = np.zeros(1, np.int32)         # an empty list is a list: a non-null pointer with n = 0 (NULL means every episode)
        Da = self.cfg.act_dim
        lo = None if low is None else np.ascontiguousarray(np.broadcast_to(np.asarray(low, np.float32), (Da,)))
        hi = None if low is None else np.ascontiguousarray(np.broadcast_to(np.asarray(high, np.float32), (Da,)))
        rows = C.c_int64()
        _lib.check(self.lib.fsrl_store_fill(self._ctx, archive._t, _ptr(ids, _i32p), n, int(first_env),
                                            int(bound_method), _ptr(lo, _f32p), _ptr(hi, _f32p), C.byref(rows)))
        return int(rows.value)

    def store_configure(self, total_size: int, buffer_num: int):
        """VectorReplayBuffer(total_size, buffer_num): re-cut the allocated store (empties it)."""
        _lib.check(self.lib.fsrl_store_configure(self._ctx, int(total_size), int(buffer_num)))

    def store_geometry(self):
        """-> (rows per sub-buffer, sub-buffers in use)"""
        sub, num = C.c_int64(), C.c_int32()
        _lib.check(self.lib.fsrl_store_geometry(self._ctx, C.byref(sub), C.byref(num)))
        return int(sub.value), int(num.value)

    def store_version(self):
        """the store's version: bumped by every push (per vector step) and every reset (fsrl_store_version)"""
        v = C.c_uint64()
        _lib.check(self.lib.fsrl_store_version(self._ctx, C.byref(v)))
        return int(v.value)

    def sample0(self):
        n = C.c_int64()
        cap = len(self)
        out = np.empty(max(cap, 1), np.int64)
        _lib.check(self.lib.fsrl_store_sample0(self._ctx, _ptr(out, _i64p), out.size, C.byref(n)))
        return out[:n.value]

    # ---------------------------------------------------------------- inference
    def actor_forward(self, obs):
        obs = np.ascontiguousarray(obs, np.float32).reshape(-1, self.cfg.obs_dim)
        k = obs.shape[0]
        mu = np.empty((k, self.cfg.act_dim), np.float32)
        sigma = np.empty((k, self.cfg.act_dim), np.float32)
        _lib.check(self.lib.fsrl_actor_forward(self._ctx, _ptr(obs, _f32p), k, _ptr(mu, _f32p),
                                               _ptr(sigma, _f32p)))
        return mu, sigma

    def actor_sample(self, obs, deterministic=False, seed=0):
        """Collector-time actions a ~ pi(.|obs): actor on the device, noise from the library RNG.
        Hot loop of the collector: staging arrays and their ctypes pointers are cached."""
        obs = np.asarray(obs, np.float32).reshape(-1, self.cfg.obs_dim)
        k = obs.shape[0]
        st = self._act_stage
        if st is None or st[0].shape[0] < k:
            cap = max(k, self.cfg.env_num)
            so, sa = np.empty((cap, self.cfg.obs_dim), np.float32), np.empty((cap, self.cfg.act_dim), np.float32)
            st = self._act_stage = (so, sa, _ptr(so, _f32p), _ptr(sa, _f32p))
        np.copyto(st[0][:k], obs)
        _lib.check(self.lib.fsrl_actor_sample(self._ctx, st[2], k, int(deterministic), int(seed), st[3]))
        return st[1][:k].copy()

    def collect_step(self, prev, obs_act, deterministic=False, bound_method=1, low=None, high=None):
        """One vector step of the collector in one C call (fsrl_collect_step): store the finished transitions `prev` =
        (env_ids, obs, act, rew, cost, terminated, truncated, obs_next) or None, and return (act, env_act, ep_rew,
        ep_len) for the observations `obs_act` (None: store only).  Staging arrays / ctypes pointers are cached."""
        Do, Da = self.cfg.obs_dim, self.cfg.act_dim
        st = self._collect_stage
        if st is None:
            cap = self.cfg.env_num
            arr = dict(ids=np.empty(cap, np.int32), obs=np.empty((cap, Do), np.float32), act=np.empty((cap, Da), np.float32),
                       rew=np.empty(cap, np.float64), cost=np.empty(cap, np.float64), term=np.empty(cap, np.uint8),
                       trunc=np.empty(cap, np.uint8), nxt=np.empty((cap, Do), np.float32), ptr=np.empty(cap, np.int64),
                       er=np.empty(cap, np.float64), el=np.empty(cap, np.int32), ei=np.empty(cap, np.int64),
                       oa=np.empty((cap, Do), np.float32), ao=np.empty((cap, Da), np.float32), eo=np.empty((cap, Da), np.float32),
                       lo=np.empty(Da, np.float32), hi=np.empty(Da, np.float32))
            types = dict(ids=_i32p, obs=_f32p, act=_f32p, rew=_f64p, cost=_f64p, term=_u8p, trunc=_u8p, nxt=_f32p, ptr=_i64p,
                         er=_f64p, el=_i32p, ei=_i64p, oa=_f32p, ao=_f32p, eo=_f32p, lo=_f32p, hi=_f32p)
            st = self._collect_stage = dict(a=arr, p={n: _ptr(arr[n], types[n]) for n in arr})
        a, p = st["a"], st["p"]
        k = 0
        if prev is not None:
            ids, obs, act, rew, cost, term, trunc, nxt = prev
            k = len(ids)
            a["ids"][:k] = ids; a["obs"][:k] = obs; a["act"][:k] = act; a["rew"][:k] = rew; a["cost"][:k] = cost
            a["term"][:k] = term; a["trunc"][:k] = trunc; a["nxt"][:k] = nxt
        ka = 0
        if obs_act is not None:
            ka = len(obs_act)
            a["oa"][:ka] = obs_act
        if low is not None:
            a["lo"][:] = low; a["hi"][:] = high
        _lib.check(self.lib.fsrl_collect_step(
            self._ctx, p["ids"], k, p["obs"], p["act"], p["rew"], p["cost"], p["term"], p["trunc"], p["nxt"], p["ptr"],
            p["er"], p["el"], p["ei"], p["oa"], ka, int(deterministic), int(bound_method),
            p["lo"] if low is not None else None, p["hi"] if low is not None else None, p["ao"], p["eo"]))
        return a["ao"][:ka].copy(), a["eo"][:ka].copy(), a["er"][:k], a["el"][:k]

    def collect_run(self, env_desc, ready, obs, act, env_act, deterministic=False, bound_method=1, low=None, high=None,
                    max_steps=1 << 30):
        """The collector's inner loop over a worker-process env in one C call (fsrl_collect_run): from the envs `ready` with
        observations `obs`, policy actions `act` and mapped actions `env_act`, step the env / store / evaluate the actor until
        a vector step finishes an episode.  -> (steps, cost_sum, obs, act, rew, cost, terminated, truncated, obs_next) where
        obs / act are the inputs of that last step and rew ... obs_next its (unstored) results."""
        Do, Da = self.cfg.obs_dim, self.cfg.act_dim
        n = len(ready)
        st = self._run_stage
        if st is None or st["n"] < n:
            cap = self.cfg.env_num
            arr = dict(ids=np.empty(cap, np.int32), obs=np.empty((cap, Do), np.float32), act=np.empty((cap, Da), np.float32),
                       eact=np.empty((cap, Da), np.float32), rew=np.empty(cap, np.float64), cost=np.empty(cap, np.float64),
                       term=np.empty(cap, np.uint8), trunc=np.empty(cap, np.uint8), nxt=np.empty((cap, Do), np.float32),
                       lo=np.empty(Da, np.float32), hi=np.empty(Da, np.float32))
            types = dict(ids=_i32p, obs=_f32p, act=_f32p, eact=_f32p, rew=_f64p, cost=_f64p, term=_u8p, trunc=_u8p, nxt=_f32p,
                         lo=_f32p, hi=_f32p)
            st = self._run_stage = dict(n=cap, a=arr, p={k: _ptr(arr[k], types[k]) for k in arr}, steps=C.c_int32(), csum=C.c_double())
        a, p = st["a"], st["p"]
        a["ids"][:n] = ready; a["obs"][:n] = obs; a["act"][:n] = act; a["eact"][:n] = env_act
        if low is not None:
            a["lo"][:] = low; a["hi"][:] = high
        _lib.check(self.lib.fsrl_collect_run(
            self._ctx, C.byref(env_desc), p["ids"], n, p["obs"], p["act"], p["eact"], int(deterministic), int(bound_method),
            p["lo"] if low is not None else None, p["hi"] if low is not None else None, int(max_steps), C.byref(st["steps"]),
            C.byref(st["csum"]), p["rew"], p["cost"], p["term"], p["trunc"], p["nxt"]))
        return (st["steps"].value, st["csum"].value, a["obs"][:n].copy(), a["act"][:n].copy(), a["rew"][:n].copy(),
                a["cost"][:n].copy(), a["term"][:n].astype(bool), a["trunc"][:n].astype(bool), a["nxt"][:n].copy())

    def collect_episodes(self, env_desc, ready, obs, n_episode, deterministic=False, bound_method=1, low=None, high=None, split=False):
        """FastCollector.collect(n_episode) over a worker-process env in ONE C call (fsrl_collect_episodes): vector steps, store,
        actor, resets, episode accounting, surplus envs.  split: the two-lane split-phase form (fsrl_collect_episodes_split).
        -> dict(steps, total_cost, terminated, truncated, ep_rews, ep_lens, t_env, t_act)"""
        Do, Da = self.cfg.obs_dim, self.cfg.act_dim
        n = len(ready)
        ids = np.ascontiguousarray(ready, np.int32)
        ob = np.ascontiguousarray(obs, np.float32).reshape(n, Do)
        lo = np.ascontiguousarray(low, np.float32) if low is not None else None
        hi = np.ascontiguousarray(high, np.float32) if low is not None else None
        steps, cost = C.c_int64(), C.c_double()
        nt, ntr, nep = C.c_int32(), C.c_int32(), C.c_int32()
        ep_rew, ep_len = np.zeros(int(n_episode), np.float64), np.zeros(int(n_episode), np.int32)
        fn = self.lib.fsrl_collect_episodes_split if split else self.lib.fsrl_collect_episodes
        _lib.check(fn(
            self._ctx, C.byref(env_desc), _ptr(ids, _i32p), n, _ptr(ob, _f32p), int(n_episode), int(deterministic), int(bound_method),
            _ptr(lo, _f32p) if lo is not None else None, _ptr(hi, _f32p) if hi is not None else None, C.byref(steps), C.byref(cost),
            C.byref(nt), C.byref(ntr), _ptr(ep_rew, _f64p), _ptr(ep_len, _i32p), C.byref(nep)))
        k = nep.value
        tm = np.zeros(2, np.float64)
        _lib.check(self.lib.fsrl_collect_timing(self._ctx, _ptr(tm, _f64p)))
        return dict(steps=int(steps.value), total_cost=float(cost.value), terminated=int(nt.value), truncated=int(ntr.value),
                    ep_rews=ep_rew[:k], ep_lens=ep_len[:k], t_env=float(tm[0]), t_act=float(tm[1]))

    # ---------------------------------------------------------------- device environments (include/fsrl_hip.h "Device environments")
    def devenv_create(self, kind, env_num, max_episode_steps, seed=0, params=(), A=None, B=None):
        """fsrl_devenv_create -> handle.  obs_dim / act_dim are the engine's; A [obs_dim, obs_dim] and B [act_dim, obs_dim] for the
        linear kind.  The envs are not reset."""
        cfg = _lib.DevEnvConfig()
        cfg.kind, cfg.env_num, cfg.obs_dim, cfg.act_dim = int(kind), int(env_num), self.cfg.obs_dim, self.cfg.act_dim
        cfg.max_episode_steps, cfg.seed = int(max_episode_steps), int(seed) & 0xFFFFFFFFFFFFFFFF
        for i, v in enumerate(params):
            cfg.p[i] = float(v)
        a = b = None
        if A is not None:
            a = np.ascontiguousarray(A, np.float32); b = np.ascontiguousarray(B, np.float32)
            assert a.shape == (self.cfg.obs_dim, self.cfg.obs_dim) and b.shape == (self.cfg.act_dim, self.cfg.obs_dim), \
                "A is [obs_dim, obs_dim], B is [act_dim, obs_dim]"
            cfg.A, cfg.B = a.ctypes.data, b.ctypes.data
        h = C.c_void_p()
        _lib.check(self.lib.fsrl_devenv_create(self._ctx, C.byref(cfg), C.byref(h)))      # copies A and B
        return h

    def devenv_destroy(self, h):
        if h:
            self.lib.fsrl_devenv_destroy(h)

    def devenv_seed(self, h, seed):
        _lib.check(self.lib.fsrl_devenv_seed(h, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def devenv_reset(self, h, env_num, ids=None):
        """-> obs of the reset envs (ids = None: all)"""
        idv = None if ids is None else np.ascontiguousarray(ids, np.int32).reshape(-1)
        n = int(env_num) if idv is None else idv.size
        obs = np.empty((n, self.cfg.obs_dim), np.float32)
        if n:
            _lib.check(self.lib.fsrl_devenv_reset(h, _ptr(idv, _i32p), n, _ptr(obs, _f32p)))
        return obs

    def devenv_step(self, h, env_num, act, ids=None):
        """-> (obs_next, rew, cost, terminated, truncated) of the listed envs (ids = None: all)"""
        idv = None if ids is None else np.ascontiguousarray(ids, np.int32).reshape(-1)
        n = int(env_num) if idv is None else idv.size
        a = np.ascontiguousarray(act, np.float32).reshape(n, self.cfg.act_dim)
        obs = np.empty((n, self.cfg.obs_dim), np.float32)
        rew, cost = np.empty(n, np.float64), np.empty(n, np.float64)
        term, trunc = np.empty(n, np.uint8), np.empty(n, np.uint8)
        if n:
            _lib.check(self.lib.fsrl_devenv_step(h, _ptr(idv, _i32p), n, _ptr(a, _f32p), _ptr(obs, _f32p), _ptr(rew, _f64p),
                                                 _ptr(cost, _f64p), _ptr(term, _u8p), _ptr(trunc, _u8p)))
        return obs, rew, cost, term.astype(bool), trunc.astype(bool)

    def devenv_get_state(self, h, env_num, state_dim):
        """-> (state [env_num, state_dim], steps of the running episode [env_num], reset ordinals [env_num])"""
        st = np.empty((int(env_num), int(state_dim)), np.float32)
        t, od = np.empty(int(env_num), np.int32), np.empty(int(env_num), np.int64)
        _lib.check(self.lib.fsrl_devenv_get_state(h, _ptr(st, _f32p), _ptr(t, _i32p), _ptr(od, _i64p)))
        return st, t, od

    def devenv_set_state(self, h, state=None, t=None, ordinal=None):
        st = None if state is None else np.ascontiguousarray(state, np.float32)
        tt = None if t is None else np.ascontiguousarray(t, np.int32)
        od = None if ordinal is None else np.ascontiguousarray(ordinal, np.int64)
        _lib.check(self.lib.fsrl_devenv_set_state(h, _ptr(st, _f32p), _ptr(tt, _i32p), _ptr(od, _i64p)))

    def collect_device(self, h, n_episode, deterministic=False, bound_method=1, low=None, high=None, max_steps_per_launch=0):
        """FastCollector.collect(n_episode) as a whole on the device (fsrl_collect_device).
        -> dict(steps, total_cost, terminated, truncated, ep_rews, ep_lens, launches)"""
        lo = np.ascontiguousarray(low, np.float32) if low is not None else None
        hi = np.ascontiguousarray(high, np.float32) if low is not None else None
        return self._collect_device(self.lib.fsrl_collect_device, h, n_episode, deterministic, bound_method, lo, hi, max_steps_per_launch)

    def evaluate_device(self, h, n_episode, deterministic=True, bound_method=1, low=None, high=None, max_steps_per_launch=0):
        """Engine.collect_device that stores nothing (fsrl_evaluate_device): FastCollector(policy, test_envs) with no buffer.  The
        same loop on the env `h`, the same result dict; the store, its books, the sampler and every random stream of the engine stay
        as they are.  Works with a trajectory archive attached, on a member of a group and with more envs than sub-buffers."""
        lo = np.ascontiguousarray(low, np.float32) if low is not None else None
        hi = np.ascontiguousarray(high, np.float32) if low is not None else None
        return self._collect_device(self.lib.fsrl_evaluate_device, h, n_episode, deterministic, bound_method, lo, hi, max_steps_per_launch)

    def collect_device_layered(self, h, n_episode, deterministic=False, bound_method=1, low=None, high=None, max_steps_per_launch=0):
        """Engine.collect_device for a LAYERED engine (hidden_sizes of any depth and width): fsrl_collect_device_layered with this one
        member.  The same arguments and result dict; the engine may be a member of any kind of group."""
        return collect_device_layered([self], [h], n_episode, deterministic, bound_method, None if low is None else [low],
                                      None if low is None else [high], max_steps_per_launch)[0]

    def evaluate_device_layered(self, h, n_episode, deterministic=True, bound_method=1, low=None, high=None, max_steps_per_launch=0):
        """Engine.evaluate_device for a LAYERED engine: fsrl_evaluate_device_layered with this one member; nothing is stored."""
        return evaluate_device_layered([self], [h], n_episode, deterministic, bound_method, None if low is None else [low],
                                       None if low is None else [high], max_steps_per_launch)[0]

    def _collect_device(self, fn, h, n_episode, deterministic, bound_method, lo, hi, max_steps_per_launch):
        steps, cost = C.c_int64(), C.c_double()
        nt, ntr, nep, nl = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        ep_rew, ep_len = np.zeros(max(int(n_episode), 1), np.float64), np.zeros(max(int(n_episode), 1), np.int32)
        _lib.check(fn(
            self._ctx, h, int(n_episode), int(bool(deterministic)), int(bound_method), _ptr(lo, _f32p), _ptr(hi, _f32p),
            int(max_steps_per_launch), C.byref(steps), C.byref(cost), C.byref(nt), C.byref(ntr), _ptr(ep_rew, _f64p),
            _ptr(ep_len, _i32p), C.byref(nep), C.byref(nl)))
        k = nep.value
        return dict(steps=int(steps.value), total_cost=float(cost.value), terminated=int(nt.value), truncated=int(ntr.value),
                    ep_rews=ep_rew[:k], ep_lens=ep_len[:k], launches=int(nl.value))

    def actor_set_resident(self, on=True, idle_timeout_us=0.0):
        """The collector's actor as a resident workgroup (include/fsrl_hip.h: fsrl_actor_set_resident); on by default."""
        _lib.check(self.lib.fsrl_actor_set_resident(self._ctx, int(bool(on)), float(idle_timeout_us)))

    def actor_release(self):
        """End the resident actor kernel now (a collect is over) instead of at the next stream work / its idle timeout."""
        self.lib.fsrl_actor_release(self._ctx)

    def actor_resident_stats(self):
        out = np.zeros(3, np.int64)
        _lib.check(self.lib.fsrl_actor_resident_stats(self._ctx, _ptr(out, _i64p)))
        return dict(launches=int(out[0]), requests=int(out[1]), live=bool(out[2]))

    def store_sizes(self, n=None):
        n = self.cfg.env_num if n is None else int(n)
        out = np.empty(n, np.int64)
        _lib.check(self.lib.fsrl_store_sizes(self._ctx, _ptr(out, _i64p), n))
        return out

    # ---------------------------------------------------------------- FOCOPS (on the PPO begin / pass / end calls)
    def focops_init(self, actor_lr=5e-4, critic_lr=1e-3, l2_reg=1e-3, delta=0.02, eta=0.02, tem_lambda=0.95,
                    max_grad_norm=0.5):
        cfg = _lib.FocopsConfig(actor_lr, critic_lr, l2_reg, delta, eta, tem_lambda, float(max_grad_norm or 0.0))
        _lib.check(self.lib.fsrl_focops_init(self._ctx, C.byref(cfg)))

    def focops_set_plan(self, four_launch: int = 0):
        """A/B and tests: 1 = the four-launch minibatch step (split-K weight gradients), 0 = three launches (default)"""
        _lib.check(self.lib.fsrl_focops_set_plan(self._ctx, int(four_launch)))

    def focops_update(self, nu, nu_loss, batch_size, repeat, perms=None, seed=0):
        """-> (stats [steps, 8]: nu_loss, nu_value, actor_loss, kl, entropy, vf0, vf1, vf_total; stopped pass or -1)."""
        _lib.check(self.lib.fsrl_focops_set_nu(self._ctx, float(nu), float(nu_loss)))
        stats, stopped = self.ppo_update([0.0], 1.0, batch_size, repeat, perms=perms, seed=seed)
        return stats[:, :_lib.FOCOPS_NSTATS], stopped

    # ---------------------------------------------------------------- PPO-Lagrangian
    def ppo_begin(self, lagrangians: Sequence[float], rescaling: float, batch_size: int) -> int:
        lag = np.ascontiguousarray(lagrangians, np.float64).reshape(-1)
        n = C.c_int64()
        _lib.check(self.lib.fsrl_ppo_begin(self._ctx, _ptr(lag, _f64p) if lag.size else None,
                                           float(rescaling), int(batch_size), C.byref(n)))
        self._n = n.value
        return n.value

    def ppo_pass(self, perm=None, seed: int = 0, wait: bool = True) -> bool:
        """One pass of minibatch steps -> True if the KL early stop fired.  wait=False only enqueues the pass (returns
        False); ppo_pass_result() then collects the verdict -- the caller can prepare the next pass meanwhile."""
        stopped = C.c_int32()
        if perm is not None:
            perm = np.ascontiguousarray(perm, np.int64)
            assert perm.size == self._n, "permutation length != batch length"
        _lib.check(self.lib.fsrl_ppo_pass(self._ctx, _ptr(perm, _i64p), int(seed), C.byref(stopped) if wait else None))
        return bool(stopped.value)

    def ppo_pass_result(self) -> bool:
        stopped = C.c_int32()
        _lib.check(self.lib.fsrl_ppo_pass_result(self._ctx, C.byref(stopped)))
        return bool(stopped.value)

    def ppo_end(self):
        n = C.c_int64()
        _lib.check(self.lib.fsrl_ppo_end(self._ctx, None, 0, C.byref(n)))  # count only: not allowed
        return n.value

    def ppo_end_stats(self, max_steps: int):
        n = C.c_int64()
        out = np.empty((max(max_steps, 1), _lib.PPO_NSTATS), np.float32)
        _lib.check(self.lib.fsrl_ppo_end(self._ctx, _ptr(out, _f32p), out.shape[0], C.byref(n)))
        return out[:n.value]

    def ppo_set_plan(self, tall_tiles: int = -1):
        """32-row tiles in the forward / backward launch of a minibatch step: -1 automatic, 0 none, n > 0 a count (A/B; same bits)"""
        _lib.check(self.lib.fsrl_ppo_set_plan(self._ctx, int(tall_tiles)))

    def ppo_set_clip_fuse(self, mode: int = -1, limit_ticks: int = -1):
        """The clipped step in two launches (clip + Adam inside the weight-gradient launch; same bits): mode -1 automatic, 0 off, 1 on;
        limit_ticks: a workgroup's longest wait in 10 ns ticks (< 0 default, 0 every workgroup gives up: the update is replayed)."""
        _lib.check(self.lib.fsrl_ppo_set_clip_fuse(self._ctx, int(mode), int(limit_ticks)))

    def ppo_clip_fuse_stats(self):
        """-> dict(available, fallbacks, steps, last_update_fused, grad_norm); between updates"""
        out = (C.c_int64 * 4)()
        gn = C.c_float()
        _lib.check(self.lib.fsrl_ppo_clip_fuse_stats(self._ctx, out, C.byref(gn)))
        return dict(available=bool(out[0]), fallbacks=int(out[1]), steps=int(out[2]), last_update_fused=bool(out[3]),
                    grad_norm=np.float32(gn.value))

    def ppo_process_stats(self):
        """process_fn of the last ppo_begin -> dict(rows_reused, rows_evaluated, equal_split, reuse): V(obs_next) rows taken from the
        V(obs) pass | evaluated by the next jobs (per critic), whether the launch ran the equal split, whether the reuse was on"""
        out = (C.c_int64 * 4)()
        _lib.check(self.lib.fsrl_ppo_process_stats(self._ctx, out))
        return dict(rows_reused=int(out[0]), rows_evaluated=int(out[1]), equal_split=bool(out[2]), reuse=bool(out[3]))

    def ppo_update(self, lagrangians, rescaling, batch_size, repeat, perms=None, seed=0):
        """-> (stats [steps, 11] float32, stopped_pass or -1)."""
        n = self.ppo_begin(lagrangians, rescaling, batch_size)
        stopped_pass = -1
        steps_per_pass = max(1, -(-n // max(batch_size, 1)))
        try:
            for k in range(repeat):
                if self.ppo_pass(None if perms is None else perms[k], seed + k if seed else 0):
                    stopped_pass = k
                    break
            stats = self.ppo_end_stats(steps_per_pass * max(repeat, 1))
        except BaseException:
            self.ppo_abort()                     # a bad permutation / HIP error must not wedge the begin ... end state
            raise
        return stats, stopped_pass

    def batch_get(self, which: str):
        n = self._n
        cols = 1 if which == "logp_old" else self.cfg.n_critics
        out = np.empty((n, cols), np.float32)
        _lib.check(self.lib.fsrl_batch_get(self._ctx, which.encode(), _ptr(out, _f32p), out.size))
        return out[:, 0] if which == "logp_old" else out

    def gae_return(self, v, v_next, rew, end_flag, gamma, gae_lambda):
        v = np.ascontiguousarray(v, np.float32); v_next = np.ascontiguousarray(v_next, np.float32)
        rew = np.ascontiguousarray(rew, np.float64)
        end = np.ascontiguousarray(end_flag).astype(np.uint8)
        out = np.empty(rew.size, np.float64)
        _lib.check(self.lib.fsrl_gae_return(self._ctx, _ptr(v, _f32p), _ptr(v_next, _f32p),
                                            _ptr(rew, _f64p), _ptr(end, _u8p), rew.size, float(gamma),
                                            float(gae_lambda), _ptr(out, _f64p)))
        return out

    def launch_floors(self, mb_rows=256, iters=200):
        """fsrl_launch_floors: {"fwdbwd", "wgrad", "adam", "triple"} in microseconds, measured now on this device."""
        out = np.zeros(4, np.float64)
        _lib.check(self.lib.fsrl_launch_floors(self._ctx, int(mb_rows), int(iters), _ptr(out, _f64p)))
        return dict(zip(("fwdbwd", "wgrad", "adam", "triple"), out.tolist()))

    def nstep_return(self, metric, end_flag, target_q, indices, gamma, n_step):
        """nstep_return (base_policy.py:543-567) on the device; target_q [bsz, ...] float32, indices [n_step, bsz]."""
        metric = np.ascontiguousarray(metric, np.float64)
        end = np.ascontiguousarray(end_flag).astype(np.uint8)
        tq = np.ascontiguousarray(target_q, np.float32)
        shape = tq.shape
        bsz = shape[0] if tq.ndim else 0
        tq2 = tq.reshape(bsz, -1) if bsz else tq.reshape(0, 1)
        idx = np.ascontiguousarray(indices, np.int64).reshape(int(n_step), bsz) if n_step >= 1 else np.zeros((0, bsz), np.int64)
        out = np.empty(tq2.shape, np.float64)
        _lib.check(self.lib.fsrl_nstep_return(self._ctx, _ptr(metric, _f64p), _ptr(end, _u8p), metric.size,
                                              _ptr(tq2, _f32p), _ptr(idx, _i64p), bsz, tq2.shape[1], float(gamma),
                                              int(n_step), _ptr(out, _f64p)))
        return out.reshape(shape)

    # ---------------------------------------------------------------- CPO / TRPO-Lagrangian
    def tr_begin(self, target_kl=0.01, backtrack_coeff=0.8, damping=0.1, l2_reg=0.0, critic_lr=1e-3,
                 max_backtracks=10, optim_critic_iters=10, cg_iters=10, norm_adv=True,
                 cost_limit=float("inf")) -> int:
        cfg = _lib.TrConfig(target_kl, backtrack_coeff, damping, l2_reg, critic_lr, max_backtracks,
                            optim_critic_iters, cg_iters, int(norm_adv),
                            cost_limit if np.isfinite(cost_limit) else 1e300)
        n = C.c_int64()
        _lib.check(self.lib.fsrl_tr_begin(self._ctx, C.byref(cfg), C.byref(n)))
        self._n = n.value
        return n.value

    @property
    def n_actor_params(self) -> int:
        return int(self.lib.fsrl_actor_param_count(self._ctx))

    def tr_linesearch_evals(self, cap=64):
        out = np.zeros(cap, np.int32)
        n = int(self.lib.fsrl_tr_linesearch_evals(self._ctx, _ptr(out, _i32p), cap))
        return out[:n]

    def tr_grad(self, which: int):
        out = np.empty(self.n_actor_params, np.float32)
        _lib.check(self.lib.fsrl_tr_grad(self._ctx, int(which), _ptr(out, _f32p), out.size))
        return out

    def tr_hvp(self, v):
        v = np.ascontiguousarray(v, np.float32)
        out = np.empty_like(v)
        _lib.check(self.lib.fsrl_tr_hvp(self._ctx, _ptr(v, _f32p), _ptr(out, _f32p), v.size))
        return out

    def tr_hvp_cached(self, v):
        """H v again at the theta / batch of the previous tr_hvp call: the cached-activation kernel of the CG solves."""
        v = np.ascontiguousarray(v, np.float32)
        out = np.empty_like(v)
        _lib.check(self.lib.fsrl_tr_hvp_cached(self._ctx, _ptr(v, _f32p), _ptr(out, _f32p), v.size))
        return out

    def tr_cg(self, rhs, damping: float, nsteps: int, tol: float):
        """The learn calls' conjugate-gradient solve on its own: (x, iterations run, last r.r) for (H + damping) x = rhs at the
        current theta, at most `nsteps` iterations, stopping once r.r < tol."""
        rhs = np.ascontiguousarray(rhs, np.float32)
        x = np.empty_like(rhs)
        iters, rs = C.c_int32(), C.c_float()
        _lib.check(self.lib.fsrl_tr_cg(self._ctx, _ptr(rhs, _f32p), rhs.size, float(damping), int(nsteps), float(tol),
                                       _ptr(x, _f32p), C.byref(iters), C.byref(rs)))
        return x, int(iters.value), float(rs.value)

    def tr_set_plan(self, tile_rows: int = 0, hvp: int = 0, wgrad: int = 0):
        """Kernel plan of the full-batch path (A/B timing, bit-identity tests); 0 / 0 = automatic.  tile_rows + 64: critic steps on the
        compute stream; + 128: read-backs by copy + stream synchronisation instead of polled completion words."""
        _lib.check(self.lib.fsrl_tr_set_plan(self._ctx, int(tile_rows), int(hvp), int(wgrad)))

    def tr_set_tile_split(self, n32_tile: int = -1, n32_hvp: int = -1):
        """A/B only: forced 32-row tile counts of the co-resident tile / cached-HVP launches (-1 = the dispatch simulation)."""
        _lib.check(self.lib.fsrl_tr_set_tile_split(self._ctx, int(n32_tile), int(n32_hvp)))

    def tr_set_co_delay(self, tile_periods: int = -1, hvp_periods: int = -1):
        """A/B only: start offset of every CU's second co-resident workgroup (periods of 8 128 cycles; -1 = default)."""
        _lib.check(self.lib.fsrl_tr_set_co_delay(self._ctx, int(tile_periods), int(hvp_periods)))

    def tr_eval(self):
        out = np.zeros(8, np.float64)
        _lib.check(self.lib.fsrl_tr_eval(self._ctx, _ptr(out, _f64p)))
        return out

    def _tr_perms(self, perms, repeat, batch_size):
        """perms: None or [repeat][N] -> (pointer or None, keep-alive array, minibatches per repeat)"""
        n = max(int(self._n), 0)
        b = max(1, min(int(batch_size), max(n, 1)))
        nmb = max(1, n // b) if n else 1                # Batch.split(merge_last=True): the remainder joins the last chunk
        if perms is None:
            return None, None, nmb
        a = np.ascontiguousarray(np.stack([np.asarray(p, np.int64) for p in perms]), np.int64)
        assert a.shape == (repeat, n), "perms must be [repeat][N]"
        return _ptr(a, _i64p), a, nmb

    def cpo_learn(self, ave_cost_return: float, repeat: int, batch_size: int = 2**31 - 1, perms=None, seed: int = 0):
        """CPO.learn (cpo.py:353-370) on the batch of the last tr_begin.  batch_size < N: Batch.split minibatches of the
        permutations `perms` ([repeat][N]; None = library shuffle), one stats row per minibatch."""
        pp, keep, nmb = self._tr_perms(perms, repeat, batch_size)
        out = np.empty((repeat * nmb, _lib.CPO_NSTATS), np.float32)
        rows = C.c_int64()
        _lib.check(self.lib.fsrl_cpo_learn_mb(self._ctx, float(ave_cost_return), int(repeat), int(min(batch_size, 2**31 - 1)), pp,
                                              int(seed), _ptr(out, _f32p), out.shape[0], C.byref(rows)))
        return out[:rows.value]

    def trpo_learn(self, lagrangians, rescaling: float, repeat: int, batch_size: int = 2**31 - 1, perms=None, seed: int = 0):
        lag = np.ascontiguousarray(lagrangians, np.float64).reshape(-1)
        pp, keep, nmb = self._tr_perms(perms, repeat, batch_size)
        out = np.empty((repeat * nmb, _lib.TRPO_NSTATS), np.float32)
        rows = C.c_int64()
        _lib.check(self.lib.fsrl_trpo_learn_mb(self._ctx, _ptr(lag, _f64p) if lag.size else None, float(rescaling), int(repeat),
                                               int(min(batch_size, 2**31 - 1)), pp, int(seed), _ptr(out, _f32p), out.shape[0],
                                               C.byref(rows)))
        return out[:rows.value]

    # ---------------------------------------------------------------- SAC-Lagrangian
    def sac_init(self, actor_lr=5e-4, critic_lr=1e-3, alpha_lr=3e-4, tau=0.05, alpha=0.005,
                 target_entropy=None, n_step=2, auto_alpha=True, use_lagrangian=True, deterministic=False,
                 exploration_sigma=0.1, unbounded=None):
        """deterministic=True selects DDPG-Lagrangian (deterministic actor + target actor, single critics).
        unbounded: ActorProb's option -- True: mu = head, False: mu = max_action * tanh(head), None: SAC-Lag's default (True)."""
        te = -float(self.cfg.act_dim) if target_entropy is None else float(target_entropy)
        cfg = _lib.SacConfig(actor_lr, critic_lr, alpha_lr, tau, alpha, te, int(n_step), int(auto_alpha),
                             int(use_lagrangian), int(deterministic), float(exploration_sigma),
                             _lib.actor_mean_code(unbounded))
        _lib.check(self.lib.fsrl_sac_init(self._ctx, C.byref(cfg)))
        self.actor_unbounded = None if deterministic else (True if unbounded is None else bool(unbounded))
        self.n_sac_actor = int(self.lib.fsrl_sac_param_count(self._ctx, 0))
        self.n_sac_critics = int(self.lib.fsrl_sac_param_count(self._ctx, 1))

    def sac_set_plan(self, plan: int = 0):
        """A/B and tests: bit 0 = split-K weight gradients at every batch size (default: the one-workgroup-per-tile kernel up to
        512 rows); bit 1 = sample and gather as two launches, bit 2 = the n-step targets as a launch of their own (default: 10
        launches per update, not 12), bit 3 = prefetch the next update's sample on the side stream (measured slower: off by default),
        bit 4 = sample + gather as a launch of their own (round 4: 10 launches; r5 default: inside the actors' forward launch, 9),
        bit 5 = no rider blocks (r6 default above 512 rows: the actor's weight-gradient launch also draws the NEXT update's batch),
        bit 6 = the critics' split-K weight-gradient launch in plain block order (r6 default: XCD-aware, 2.3x less memory-side traffic)"""
        _lib.check(self.lib.fsrl_sac_set_plan(self._ctx, int(plan)))

    def sac_set_params(self, actor_flat, critics_flat, log_alpha=0.0):
        a = np.ascontiguousarray(actor_flat, np.float32); c = np.ascontiguousarray(critics_flat, np.float32)
        _lib.check(self.lib.fsrl_sac_params_set(self._ctx, _ptr(a, _f32p), a.size, _ptr(c, _f32p), c.size,
                                                float(log_alpha)))

    def sac_put_params(self, which: int, flat):
        """Overwrite one parameter set (0 actor, 1 critics, 2 critics_old, 3 actor_old); nothing else changes."""
        a = np.ascontiguousarray(flat, np.float32)
        _lib.check(self.lib.fsrl_sac_params_put(self._ctx, int(which), _ptr(a, _f32p), a.size))

    def sac_get_params(self, which: int):
        """which: 0 actor, 1 critics, 2 critics_old, 3 actor_old (DDPG-Lag) -> (flat params, alpha)."""
        out = np.empty(self.n_sac_actor if which in (0, 3) else self.n_sac_critics, np.float32)
        alpha = C.c_float()
        _lib.check(self.lib.fsrl_sac_params_get(self._ctx, int(which), _ptr(out, _f32p), out.size, C.byref(alpha)))
        return out, float(alpha.value)

    def sac_update(self, batch_size, lagrangians, rescaling, indices=None, eps_target=None, eps_pi=None, seed=0,
                   sync=True):
        """One SAC-Lag update.  indices/eps_* given together = caller RNG (parity); all None = device
        RNG.  sync=False only enqueues the work: the statistics row is fetched later by sac_drain()."""
        lag = np.ascontiguousarray(lagrangians, np.float64).reshape(-1)
        idx = None if indices is None else np.ascontiguousarray(indices, np.int64)
        et = None if eps_target is None else np.ascontiguousarray(eps_target, np.float32)
        ep = None if eps_pi is None else np.ascontiguousarray(eps_pi, np.float32)
        if idx is not None:
            assert idx.size == batch_size
        out = np.empty(_lib.SAC_NSTATS, np.float32) if sync else None
        _lib.check(self.lib.fsrl_sac_update(self._ctx, int(batch_size), _ptr(idx, _i64p), _ptr(et, _f32p),
                                            _ptr(ep, _f32p), int(seed), _ptr(lag, _f64p) if lag.size else None,
                                            float(rescaling), _ptr(out, _f32p)))
        return out

    def sac_drain(self, max_rows=4096):
        """Statistics rows [n, SAC_NSTATS] of the sync=False updates since the last drain."""
        out = np.empty((int(max_rows), getattr(self, "_ring_cols", _lib.SAC_NSTATS)), np.float32)
        n = int(self.lib.fsrl_sac_stats_drain(self._ctx, _ptr(out, _f32p), int(max_rows)))
        if n < 0:
            _lib.check(n)
        return out[:n]

    def sac_last_sample(self, batch_size):
        idx = np.empty(int(batch_size), np.int64)
        et = np.empty((int(batch_size), self.cfg.act_dim), np.float32); ep = np.empty_like(et)
        _lib.check(self.lib.fsrl_sac_last_sample(self._ctx, _ptr(idx, _i64p), _ptr(et, _f32p), _ptr(ep, _f32p),
                                                 int(batch_size)))
        return idx, et, ep

    def sac_last_chain(self, batch_size, n_step):
        """n-step chains [n_step][B] and end bits of the last sac_update's sample"""
        ch = np.empty((int(n_step), int(batch_size)), np.int64); end = np.empty(ch.shape, np.uint8)
        _lib.check(self.lib.fsrl_sac_last_chain(self._ctx, _ptr(ch, _i64p), _ptr(end, _u8p), int(batch_size)))
        return ch, end

    # ---------------------------------------------------------------- prioritised replay (SAC-Lag / DDPG-Lag contexts, solo or grouped)
    def per_enable(self, alpha, beta, weight_norm=True):
        """tianshou PrioritizedReplayBuffer's sum tree over this context's store, on the device (include/fsrl_hip.h)"""
        _lib.check(self.lib.fsrl_per_enable(self._ctx, float(alpha), float(beta), int(bool(weight_norm))))
        self.per_on = True

    def per_set_beta(self, beta):
        _lib.check(self.lib.fsrl_per_set_beta(self._ctx, float(beta)))

    def per_update_weight(self, indices, weights):
        idx = np.ascontiguousarray(indices, np.int64).reshape(-1)
        w = np.ascontiguousarray(weights, np.float64).reshape(-1)
        assert idx.size == w.size
        _lib.check(self.lib.fsrl_per_update_weight(self._ctx, _ptr(idx, _i64p), _ptr(w, _f64p), idx.size))

    def per_state(self, leaves=True):
        """(leaves float64 [buffer_num * sub_size] or None, max_prio, min_prio, total)"""
        sub, num = self.store_geometry()
        out = np.empty(sub * num, np.float64) if leaves else None
        mx, mn, tot = C.c_double(), C.c_double(), C.c_double()
        _lib.check(self.lib.fsrl_per_state(self._ctx, _ptr(out, _f64p), 0 if out is None else out.size, C.byref(mx), C.byref(mn),
                                           C.byref(tot)))
        return out, mx.value, mn.value, tot.value

    def per_last_weights(self, batch_size):
        out = np.empty(int(batch_size), np.float32)
        _lib.check(self.lib.fsrl_per_last_weights(self._ctx, _ptr(out, _f32p), int(batch_size)))
        return out

    def per_last_td(self, batch_size):
        out = np.empty(int(batch_size), np.float32)
        _lib.check(self.lib.fsrl_per_last_td(self._ctx, _ptr(out, _f32p), int(batch_size)))
        return out

    def sac_actor_forward(self, obs):
        obs = np.ascontiguousarray(obs, np.float32).reshape(-1, self.cfg.obs_dim)
        k = obs.shape[0]
        mu = np.empty((k, self.cfg.act_dim), np.float32); sigma = np.empty_like(mu)
        _lib.check(self.lib.fsrl_sac_actor_forward(self._ctx, _ptr(obs, _f32p), k, _ptr(mu, _f32p),
                                                   _ptr(sigma, _f32p)))
        return mu, sigma

    # ---------------------------------------------------------------- CVPO (on the SAC replay context)
    def cvpo_init(self, qc_thres, actor_lr=5e-4, critic_lr=1e-3, tau=0.05, n_step=2, double_critic=False,
                  sample_act_num=16, estep_iter_num=1, mstep_iter_num=1, estep_kl=0.02, estep_dual_max=20.0,
                  estep_dual_lr=0.02, mstep_kl_mu=0.005, mstep_kl_std=0.0005, mstep_dual_max=0.5, mstep_dual_lr=0.1,
                  unbounded=None):
        """fsrl_cvpo_init (cvpo.py:71-163).  Parameters then move through the sac_* accessors (which=3: actor_old).
        unbounded: ActorProb's option -- True: mu = head, False: mu = max_action * tanh(head), None: CVPO's default (False)."""
        cfg = _lib.CvpoConfig(actor_lr, critic_lr, tau, int(n_step), int(double_critic), int(sample_act_num),
                              int(estep_iter_num), int(mstep_iter_num), estep_kl, estep_dual_max, estep_dual_lr,
                              mstep_kl_mu, mstep_kl_std, mstep_dual_max, mstep_dual_lr, float(qc_thres),
                              _lib.actor_mean_code(unbounded))
        _lib.check(self.lib.fsrl_cvpo_init(self._ctx, C.byref(cfg)))
        self.actor_unbounded = False if unbounded is None else bool(unbounded)
        self.n_sac_actor = int(self.lib.fsrl_sac_param_count(self._ctx, 0))
        self.n_sac_critics = int(self.lib.fsrl_sac_param_count(self._ctx, 1))
        self._ring_cols = _lib.CVPO_NSTATS
        self._cvpo_k = int(sample_act_num)

    def cvpo_pre_update(self):
        _lib.check(self.lib.fsrl_cvpo_pre_update(self._ctx))

    def cvpo_post_update(self):
        _lib.check(self.lib.fsrl_cvpo_post_update(self._ctx))

    def cvpo_set_thres(self, qc_thres):
        _lib.check(self.lib.fsrl_cvpo_set_thres(self._ctx, float(qc_thres)))

    def cvpo_update(self, batch_size, indices=None, eps_target=None, eps_particles=None, seed=0, sync=True):
        """One CVPO.update.  indices / eps_target [B,Da] / eps_particles [K,B,Da] together = caller RNG; all None =
        device RNG.  sync=False only enqueues; rows come back through sac_drain()."""
        idx = None if indices is None else np.ascontiguousarray(indices, np.int64)
        et = None if eps_target is None else np.ascontiguousarray(eps_target, np.float32)
        ek = None if eps_particles is None else np.ascontiguousarray(eps_particles, np.float32)
        if idx is not None:
            assert idx.size == batch_size and et.size == batch_size * self.cfg.act_dim
            assert ek.size == self._cvpo_k * batch_size * self.cfg.act_dim
        out = np.empty(_lib.CVPO_NSTATS, np.float32) if sync else None
        _lib.check(self.lib.fsrl_cvpo_update(self._ctx, int(batch_size), _ptr(idx, _i64p), _ptr(et, _f32p),
                                             _ptr(ek, _f32p), int(seed), _ptr(out, _f32p)))
        return out

    def cvpo_duals(self):
        """(eta, lambda, mstep_dual_mu, mstep_dual_std)"""
        out = np.empty(4, np.float32)
        _lib.check(self.lib.fsrl_cvpo_duals_get(self._ctx, _ptr(out, _f32p)))
        return out

    def cvpo_last_particles(self, batch_size):
        out = np.empty((self._cvpo_k, int(batch_size), self.cfg.act_dim), np.float32)
        _lib.check(self.lib.fsrl_cvpo_last_particles(self._ctx, _ptr(out, _f32p), out.size))
        return out

    # ---------------------------------------------------------------- metric exchange (RCCL through the C ABI)
    def comm_unique_id(self) -> bytes:
        buf = np.zeros(128, np.uint8)
        _lib.check(self.lib.fsrl_comm_unique_id(_ptr(buf, _u8p), 128))
        return buf.tobytes()

    def comm_init(self, rank: int, world: int, uid: bytes):
        buf = np.frombuffer(uid, np.uint8).copy()
        _lib.check(self.lib.fsrl_comm_init(self._ctx, int(rank), int(world), _ptr(buf, _u8p), buf.size))

    def comm_init_from_torch(self):
        """Join the library's own RCCL communicator using the process group torch.distributed already has (any backend,
        gloo included) only to hand rank 0's 128-byte id around; afterwards fsrl_metrics_allreduce needs torch no more."""
        import torch.distributed as dist
        assert dist.is_initialized(), "init a torch.distributed process group first (it only carries the id)"
        rank, world = dist.get_rank(), dist.get_world_size()
        box = [self.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        self.comm_init(rank, world, box[0])

    def comm_info(self):
        r, w = C.c_int32(), C.c_int32()
        _lib.check(self.lib.fsrl_comm_info(self._ctx, C.byref(r), C.byref(w)))
        return int(r.value), int(w.value)

    def metrics_allreduce(self, vec):
        """Element-wise sum of a float64 vector (<= 64 entries) over the ranks; the identity without a communicator."""
        v = np.ascontiguousarray(vec, np.float64).copy()
        _lib.check(self.lib.fsrl_metrics_allreduce(self._ctx, _ptr(v, _f64p), v.size))
        return v

    def comm_destroy(self):
        _lib.check(self.lib.fsrl_comm_destroy(self._ctx))

    def set_profiling(self, on: bool):
        _lib.check(self.lib.fsrl_set_profiling(self._ctx, int(on)))

    def last_timing(self):
        out = np.zeros(5, np.float64)
        _lib.check(self.lib.fsrl_last_timing(self._ctx, _ptr(out, _f64p), 5))
        return dict(process_ms=out[0], learn_ms=out[1], fwdbwd_ms=out[2], fwdbwd_launches=int(out[3]),
                    fwdbwd_raw_ms=out[4])


TRAJ_COLUMNS = ("observations", "next_observations", "actions", "rewards", "costs", "terminals", "timeouts")
TRAJ_COUNTERS = ("committed", "rejected_window", "dropped_long", "compactions", "rows", "refused_full", "episodes", "launches",
                 "h2d_bytes", "abandoned", "import_open", "fill_launches", "fill_copies")


class TrajArchive:
    """One fsrl_traj (include/fsrl_hip.h): finished episodes of the engines that feed it, in HBM, in the DSRL column layout.
    Plumbing like Engine: every method forwards to one entry point.  fsrl_amd.data.TrajectoryBuffer puts the reference's
    semantics on top."""

    def __init__(self, engine: "Engine", max_rows: int, max_episodes: int, max_episode_len: int, bound_method: int = 1,
                 low=None, high=None):
        self.lib = engine.lib
        self.obs_dim, self.act_dim = engine.cfg.obs_dim, engine.cfg.act_dim
        self.max_rows, self.max_episodes, self.max_episode_len = int(max_rows), int(max_episodes), int(max_episode_len)
        lo = None if low is None else np.ascontiguousarray(np.broadcast_to(np.asarray(low, np.float32), (self.act_dim,)))
        hi = None if low is None else np.ascontiguousarray(np.broadcast_to(np.asarray(high, np.float32), (self.act_dim,)))
        self._t = C.c_void_p()
        _lib.check(self.lib.fsrl_traj_create(engine._ctx, self.max_rows, self.max_episodes, self.max_episode_len, int(bound_method),
                                             _ptr(lo, _f32p), _ptr(hi, _f32p), C.byref(self._t)))

    def close(self):
        if getattr(self, "_t", None) is not None and self._t:
            self.lib.fsrl_traj_destroy(self._t)
            self._t = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def attach(self, engine: "Engine") -> int:
        """-> the source number the episodes of `engine` carry"""
        src = C.c_int32()
        _lib.check(self.lib.fsrl_traj_attach(self._t, engine._ctx, C.byref(src)))
        return int(src.value)

    def detach(self, engine: "Engine") -> None:
        _lib.check(self.lib.fsrl_traj_detach(self._t, engine._ctx))

    def abandon(self, engine: "Engine") -> None:
        """the open episodes of `engine` are discarded: its envs were reset in mid-episode"""
        _lib.check(self.lib.fsrl_traj_abandon(self._t, engine._ctx))

    def set_window(self, rmin, rmax, cmin, cmax):
        _lib.check(self.lib.fsrl_traj_set_window(self._t, float(rmin), float(rmax), float(cmin), float(cmax)))

    def flush(self):
        _lib.check(self.lib.fsrl_traj_flush(self._t))

    def episodes(self):
        """-> (ids, rows, reward returns, cost returns, sources) of the alive episodes in table order, as of the last flush"""
        n = C.c_int64()
        _lib.check(self.lib.fsrl_traj_episodes(self._t, 0, None, None, None, None, None, C.byref(n)))
        k = max(int(n.value), 1)
        ids, rows, src = np.empty(k, np.int32), np.empty(k, np.int32), np.empty(k, np.int32)
        rew, cost = np.empty(k, np.float64), np.empty(k, np.float64)
        _lib.check(self.lib.fsrl_traj_episodes(self._t, k, _ptr(ids, _i32p), _ptr(rows, _i32p), _ptr(rew, _f64p), _ptr(cost, _f64p),
                                               _ptr(src, _i32p), C.byref(n)))
        k = int(n.value)
        return ids[:k], rows[:k], rew[:k], cost[:k], src[:k]

    def keep(self, ids):
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        _lib.check(self.lib.fsrl_traj_keep(self._t, _ptr(ids, _i32p) if ids.size else None, ids.size))

    def replace(self, victim_id: int):
        _lib.check(self.lib.fsrl_traj_replace(self._t, int(victim_id)))

    def export(self):
        """-> dict of the seven DSRL columns (numpy), alive episodes in table order"""
        n = C.c_int64()
        _lib.check(self.lib.fsrl_traj_export(self._t, None, None, None, None, None, None, None, 0, C.byref(n)))
        k = int(n.value)
        out = dict(observations=np.empty((k, self.obs_dim), np.float32), next_observations=np.empty((k, self.obs_dim), np.float32),
                   actions=np.empty((k, self.act_dim), np.float32), rewards=np.empty(k, np.float64), costs=np.empty(k, np.float64),
                   terminals=np.empty(k, np.uint8), timeouts=np.empty(k, np.uint8))
        if k:
            _lib.check(self.lib.fsrl_traj_export(
                self._t, _ptr(out["observations"], _f32p), _ptr(out["next_observations"], _f32p), _ptr(out["actions"], _f32p),
                _ptr(out["rewards"], _f64p), _ptr(out["costs"], _f64p), _ptr(out["terminals"], _u8p), _ptr(out["timeouts"], _u8p),
                k, C.byref(n)))
        out["terminals"] = out["terminals"].astype(bool); out["timeouts"] = out["timeouts"].astype(bool)
        return out

    def import_rows(self, data, source: int = 0):
        """fsrl_traj_import: host columns in the export layout (a dict with the TRAJ_COLUMNS keys) -> (episodes accepted, rows
        accepted).  Episodes end where terminals | timeouts is set; a trailing open run is dropped; every episode is committed as
        a tapped one is (window, max_episode_len, room).  MemoryError when one found no room: the others are in."""
        obs = np.ascontiguousarray(data["observations"], np.float32)
        k = obs.shape[0]
        obs = obs.reshape(k, -1)
        nxt = np.ascontiguousarray(data["next_observations"], np.float32).reshape(k, -1)
        act = np.ascontiguousarray(data["actions"], np.float32).reshape(k, -1)
        assert k == 0 or (obs.shape[1] == self.obs_dim and nxt.shape[1] == self.obs_dim), \
            f"obs_dim: the dataset has {obs.shape[1]}, the trajectory archive {self.obs_dim}"
        assert k == 0 or act.shape[1] == self.act_dim, f"act_dim: the dataset has {act.shape[1]}, the trajectory archive {self.act_dim}"
        rew = np.ascontiguousarray(data["rewards"], np.float64).reshape(-1)
        cost = np.ascontiguousarray(data["costs"], np.float64).reshape(-1)
        term = np.ascontiguousarray(np.asarray(data["terminals"]) != 0, np.uint8).reshape(-1)
        tout = np.ascontiguousarray(np.asarray(data["timeouts"]) != 0, np.uint8).reshape(-1)
        assert rew.size == k and cost.size == k and term.size == k and tout.size == k and len(nxt) == k and len(act) == k, \
            "the dataset's columns differ in length"
        ne, nr = C.c_int64(), C.c_int64()
        self.last_import = (0, 0)
        rc = self.lib.fsrl_traj_import(self._t, k, _ptr(obs, _f32p), _ptr(nxt, _f32p), _ptr(act, _f32p), _ptr(rew, _f64p),
                                       _ptr(cost, _f64p), _ptr(term, _u8p), _ptr(tout, _u8p), int(source), C.byref(ne), C.byref(nr))
        self.last_import = (int(ne.value), int(nr.value))      # also when the call reports an episode without room
        _lib.check(rc)
        return self.last_import

    def clear(self):
        _lib.check(self.lib.fsrl_traj_clear(self._t))

    def counters(self) -> dict:
        out = np.zeros(len(TRAJ_COUNTERS), np.int64)
        _lib.check(self.lib.fsrl_traj_counters(self._t, _ptr(out, _i64p), out.size))
        return dict(zip(TRAJ_COUNTERS, (int(v) for v in out)))


def evaluate_device_group(engines, env_handles, n_episodes, deterministic=True, bound_method=1, lows=None, highs=None,
                          max_steps_per_launch=0):
    """Engine.evaluate_device for k engines in ONE looping launch per max_steps_per_launch vector steps (fsrl_evaluate_device_group):
    member i's result and env state are Engine.evaluate_device's on it, bit for bit; nothing of any member's store moves.
    Arguments and result as collect_device_group."""
    return collect_device_group(engines, env_handles, n_episodes, deterministic, bound_method, lows, highs, max_steps_per_launch, _store=False)


def collect_device_layered(engines, env_handles, n_episodes, deterministic=False, bound_method=1, lows=None, highs=None,
                           max_steps_per_launch=0):
    """collect_device_group for LAYERED engines (fsrl_collect_device_layered): k members' whole collects in one looping launch of the
    layered collect kernel, one workgroup per member; one member is the solo collect.  The members share hidden_sizes and may sit in
    any kind of group or in none.  Arguments and result as collect_device_group."""
    return collect_device_group(engines, env_handles, n_episodes, deterministic, bound_method, lows, highs, max_steps_per_launch,
                                _fn="fsrl_collect_device_layered")


def evaluate_device_layered(engines, env_handles, n_episodes, deterministic=True, bound_method=1, lows=None, highs=None,
                            max_steps_per_launch=0):
    """evaluate_device_group for LAYERED engines (fsrl_evaluate_device_layered): collect_device_layered that stores nothing."""
    return collect_device_group(engines, env_handles, n_episodes, deterministic, bound_method, lows, highs, max_steps_per_launch,
                                _fn="fsrl_evaluate_device_layered")


def collect_device_group(engines, env_handles, n_episodes, deterministic=False, bound_method=1, lows=None, highs=None,
                         max_steps_per_launch=0, _store=True, _fn=None):
    """Engine.collect_device for k engines in ONE looping launch per max_steps_per_launch vector steps (fsrl_collect_device_group):
    member i's collect is Engine.collect_device on it, bit for bit.  The engines may be ungrouped or members of any kind of group.
    env_handles: each engine's devenv handle; n_episodes: one count or one per member; lows / highs: None or one row per member.
    -> one dict per member with the keys of Engine.collect_device (`launches` is the call's)."""
    engines = list(engines)
    k = len(engines)
    assert len(env_handles) == k, "one device env per engine"
    n_ep = np.ascontiguousarray(np.broadcast_to(np.asarray(n_episodes, np.int32), (k,)) if k else np.zeros(0, np.int32))
    lib = engines[0].lib if k else _lib.load()
    ctxs = (C.c_void_p * max(k, 1))(*[e._ctx for e in engines])
    envs = (C.c_void_p * max(k, 1))(*[h if isinstance(h, C.c_void_p) else C.c_void_p(h) for h in env_handles])
    lo = hi = None
    if lows is not None and k:
        Da = engines[0].cfg.act_dim
        lo = np.ascontiguousarray(np.asarray(lows, np.float32).reshape(k, Da))
        hi = np.ascontiguousarray(np.asarray(highs, np.float32).reshape(k, Da))
    off = np.concatenate([[0], np.cumsum(np.maximum(n_ep, 0), dtype=np.int64)])
    tot = max(int(off[-1]), 1)
    steps, cost = np.zeros(max(k, 1), np.int64), np.zeros(max(k, 1), np.float64)
    nt, ntr, nep = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int32)
    ep_rew, ep_len = np.zeros(tot, np.float64), np.zeros(tot, np.int32)
    nl = C.c_int32()
    _lib.check(getattr(lib, _fn or ("fsrl_collect_device_group" if _store else "fsrl_evaluate_device_group"))(
        ctxs, envs, k, _ptr(n_ep, _i32p), int(bool(deterministic)), int(bound_method), _ptr(lo, _f32p), _ptr(hi, _f32p),
        int(max_steps_per_launch), _ptr(steps, _i64p), _ptr(cost, _f64p), _ptr(nt, _i32p), _ptr(ntr, _i32p), _ptr(ep_rew, _f64p),
        _ptr(ep_len, _i32p), _ptr(nep, _i32p), C.byref(nl)))
    return [dict(steps=int(steps[i]), total_cost=float(cost[i]), terminated=int(nt[i]), truncated=int(ntr[i]),
                 ep_rews=ep_rew[off[i]:off[i] + nep[i]].copy(), ep_lens=ep_len[off[i]:off[i] + nep[i]].copy(), launches=int(nl.value))
            for i in range(k)]


class _NativeGroup:
    """`engines`, `lib` and the native handle `_g` of a group made by `<_symbols>_create` and freed by `<_symbols>_destroy`"""
    _symbols = ""                       # the C ABI prefix of the group: fsrl_group, fsrl_sac_group, ...

    def __init__(self, engines):
        self.engines = list(engines)
        assert self.engines, "a group needs at least one engine"
        self.lib = self.engines[0].lib
        k = len(self.engines)
        arr = (C.c_void_p * k)(*[e._ctx for e in self.engines])
        self._g = C.c_void_p()
        _lib.check(getattr(self.lib, self._symbols + "_create")(arr, k, C.byref(self._g)))

    def close(self):
        if getattr(self, "_g", None) is not None and self._g:
            getattr(self.lib, self._symbols + "_destroy")(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _LockStepCollect(_NativeGroup):
    """collect_step of an object that owns `engines`, a native group handle `_g` and a `_collect_step_symbol` with
    fsrl_group_collect_step's signature: the staging arrays and the call, shared by EngineGroup and EngineCollectGroup, and the
    three `<_symbols>_actor_*` calls of the group's resident collect kernel."""
    _collect_stage = None               # cached staging arrays + ctypes pointers of collect_step

    def collect_step(self, prevs, obs_acts, deterministic=False, bound_method=1, low=None, high=None):
        """Engine.collect_step on every member in ONE call with ONE actor request (fsrl_group_collect_step for an EngineGroup,
        fsrl_collect_group_step for an EngineCollectGroup).  prevs / obs_acts: per member what Engine.collect_step takes (None
        allowed); low / high: None, one array for every member or a per-member list.
        -> per member (act, env_act, ep_rew, ep_len), as Engine.collect_step.  Staging arrays / ctypes pointers are cached."""
        engs = self.engines
        n = len(engs)
        Do, Da = engs[0].cfg.obs_dim, engs[0].cfg.act_dim
        st = self._collect_stage
        if st is None:
            cap = sum(e.cfg.env_num for e in engs)
            arr = dict(ids=np.empty(cap, np.int32), obs=np.empty((cap, Do), np.float32), act=np.empty((cap, Da), np.float32),
                       rew=np.empty(cap, np.float64), cost=np.empty(cap, np.float64), term=np.empty(cap, np.uint8),
                       trunc=np.empty(cap, np.uint8), nxt=np.empty((cap, Do), np.float32), ptr=np.empty(cap, np.int64),
                       er=np.empty(cap, np.float64), el=np.empty(cap, np.int32), ei=np.empty(cap, np.int64),
                       oa=np.empty((cap, Do), np.float32), ao=np.empty((cap, Da), np.float32), eo=np.empty((cap, Da), np.float32),
                       lo=np.empty((n, Da), np.float32), hi=np.empty((n, Da), np.float32), k=np.empty(n, np.int32),
                       ka=np.empty(n, np.int32))
            types = dict(ids=_i32p, obs=_f32p, act=_f32p, rew=_f64p, cost=_f64p, term=_u8p, trunc=_u8p, nxt=_f32p, ptr=_i64p,
                         er=_f64p, el=_i32p, ei=_i64p, oa=_f32p, ao=_f32p, eo=_f32p, lo=_f32p, hi=_f32p, k=_i32p, ka=_i32p)
            st = self._collect_stage = dict(a=arr, p={m: _ptr(arr[m], types[m]) for m in arr})
        a, p = st["a"], st["p"]
        ks, kas = a["k"], a["ka"]
        o = 0
        for i, prev in enumerate(prevs):
            k = 0
            if prev is not None:
                ids, obs, act, rew, cost, term, trunc, nxt = prev
                k = len(ids)
                a["ids"][o:o + k] = ids; a["obs"][o:o + k] = obs; a["act"][o:o + k] = act; a["rew"][o:o + k] = rew
                a["cost"][o:o + k] = cost; a["term"][o:o + k] = term; a["trunc"][o:o + k] = trunc; a["nxt"][o:o + k] = nxt
            ks[i] = k
            o += k
        o = 0
        for i, oa in enumerate(obs_acts):
            ka = 0 if oa is None else len(oa)
            if ka:
                a["oa"][o:o + ka] = oa
            kas[i] = ka
            o += ka
        if low is not None:
            a["lo"][:] = np.asarray(low, np.float32).reshape(-1, Da); a["hi"][:] = np.asarray(high, np.float32).reshape(-1, Da)
        _lib.check(getattr(self.lib, self._collect_step_symbol)(
            self._g, p["k"], p["ids"], p["obs"], p["act"], p["rew"], p["cost"], p["term"], p["trunc"], p["nxt"], p["ptr"],
            p["er"], p["el"], p["ei"], p["ka"], p["oa"], int(deterministic), int(bound_method),
            p["lo"] if low is not None else None, p["hi"] if low is not None else None, p["ao"], p["eo"]))
        out, o, oa_ = [], 0, 0
        for i in range(n):
            k, ka = int(ks[i]), int(kas[i])
            out.append((a["ao"][oa_:oa_ + ka].copy(), a["eo"][oa_:oa_ + ka].copy(), a["er"][o:o + k], a["el"][o:o + k]))
            o += k; oa_ += ka
        return out

    def collect_episodes(self, env_descs, readys, obs, n_episodes, deterministic=False, bound_method=1, low=None, high=None):
        """GroupCollector.collect(n_episode) over worker-process envs in ONE C call (fsrl_group_collect_episodes for an EngineGroup,
        fsrl_collect_episodes_group for an EngineCollectGroup): Engine.collect_episodes of every member, the members' envs stepped
        together, one collect_step per vector step.  env_descs / readys / obs / n_episodes: one entry per member; low / high: None,
        one array for every member or a per-member list.
        -> per member dict(steps, total_cost, terminated, truncated, ep_rews, ep_lens, t_env, t_act) (t_*: the group's).
        An error carries `failed_member`: the member an argument error names, or the one whose env failed (-1: none)."""
        engs = self.engines
        k = len(engs)
        assert len(env_descs) == k and len(readys) == k and len(obs) == k and len(n_episodes) == k, "one entry per member"
        Do, Da = engs[0].cfg.obs_dim, engs[0].cfg.act_dim
        descs = (C.POINTER(_lib.ShmEnv) * k)(*[C.pointer(d) for d in env_descs])
        n = np.array([len(r) for r in readys], np.int32)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(r, np.int32).reshape(-1) for r in readys]), np.int32)
        ob = np.ascontiguousarray(np.concatenate([np.asarray(o, np.float32).reshape(len(r), -1) for o, r in zip(obs, readys)]), np.float32)
        assert ob.shape[1] == Do, "obs: [n_i][obs_dim] per member"
        ne = np.array([int(x) for x in n_episodes], np.int32)
        lo = hi = None
        if low is not None:
            lo = np.empty((k, Da), np.float32); hi = np.empty((k, Da), np.float32)
            lo[:] = np.asarray(low, np.float32).reshape(-1, Da); hi[:] = np.asarray(high, np.float32).reshape(-1, Da)
        steps, cost = np.zeros(k, np.int64), np.zeros(k, np.float64)
        nt, ntr, nep = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.int32)
        cap = int(np.maximum(ne, 0).sum())
        ep_rew, ep_len = np.zeros(max(cap, 1), np.float64), np.zeros(max(cap, 1), np.int32)
        tm = np.zeros(2, np.float64)
        failed = C.c_int32(-1)
        rc = getattr(self.lib, self._collect_episodes_symbol)(
            self._g, descs, _ptr(n, _i32p), _ptr(ids, _i32p), _ptr(ob, _f32p), _ptr(ne, _i32p), int(deterministic), int(bound_method),
            _ptr(lo, _f32p) if lo is not None else None, _ptr(hi, _f32p) if hi is not None else None, _ptr(steps, _i64p),
            _ptr(cost, _f64p), _ptr(nt, _i32p), _ptr(ntr, _i32p), _ptr(ep_rew, _f64p), _ptr(ep_len, _i32p), _ptr(nep, _i32p),
            _ptr(tm, _f64p), C.byref(failed))
        try:
            _lib.check(rc)
        except BaseException as e:
            e.failed_member = int(failed.value)
            raise
        out, off = [], 0
        for i in range(k):
            j = int(nep[i])
            out.append(dict(steps=int(steps[i]), total_cost=float(cost[i]), terminated=int(nt[i]), truncated=int(ntr[i]),
                            ep_rews=ep_rew[off:off + j].copy(), ep_lens=ep_len[off:off + j].copy(), t_env=float(tm[0]),
                            t_act=float(tm[1])))
            off += int(ne[i])
        return out

    def collect_step_outputs(self):
        """(ptr, ep_idx) of the rows the last collect_step stored, concatenated over members (views of the staging arrays)."""
        a = self._collect_stage["a"]
        k = int(a["k"].sum())
        return a["ptr"][:k], a["ei"][:k]

    def actor_set_resident(self, on=True, idle_timeout_us=0.0):
        """The group's resident collect kernel (include/fsrl_hip.h: fsrl_group_actor_set_resident,
        fsrl_collect_group_actor_set_resident); on by default."""
        _lib.check(getattr(self.lib, self._symbols + "_actor_set_resident")(self._g, int(bool(on)), float(idle_timeout_us)))

    def actor_release(self):
        """End the group's resident collect kernel now (a grouped collect is over)."""
        if getattr(self, "_g", None) is not None and self._g:
            getattr(self.lib, self._symbols + "_actor_release")(self._g)

    def actor_resident_stats(self):
        out = np.zeros(3, np.int64)
        _lib.check(getattr(self.lib, self._symbols + "_actor_resident_stats")(self._g, _ptr(out, _i64p)))
        return dict(launches=int(out[0]), requests=int(out[1]), live=bool(out[2]))


class EngineGroup(_LockStepCollect):
    """k PPO-Lagrangian engines, or k FOCOPS engines (focops_init), of one network shape on one GPU, updated in lock step
    (fsrl_group_*): every launch of the minibatch step carries all members.  Members keep their own store, parameters and
    random streams; use the engines as usual for everything else (push, collect_step, get_params ...).
    A PPO-Lagrangian group may be a sweep: its members agree on the network shape, n_critics, max_action, unbounded and on whether
    max_grad_norm is on, and may differ in every other hyper-parameter (eps_clip, dual_clip, vf_coef, the max_grad_norm value,
    target_kl, norm_adv, use_lagrangian, rew_norm, value_clip, lr, beta1, beta2, adam_eps); ppo_update_each adds a minibatch size and a
    number of passes per member.  A FOCOPS group keeps one set of hyper-parameters (learning rates may differ).
    The members may all be layered contexts of one `hidden_sizes` and `force_layered`: the group then runs the layered step,
    2 L + 5 launches for all members, bit-identical per member to Engine.ppo_update / Engine.focops_update at every group size
    (a layered FOCOPS group has no tile-height plan to differ in); collect_step is one sequence of L + 2
    launches for all members instead of a resident kernel (actor_resident_stats counts those sequences, `live` stays False;
    actor_set_resident(False) selects the member-by-member calls; set_plan is accepted and has no effect)."""

    _symbols = "fsrl_group"
    _collect_step_symbol = "fsrl_group_collect_step"
    _collect_episodes_symbol = "fsrl_group_collect_episodes"

    def set_plan(self, tall_tiles=-1):
        """32-row tiles per (member, network) in the forward / backward launch: -1 automatic, 0 none, n > 0 a count (A/B; same bits)."""
        _lib.check(self.lib.fsrl_group_set_plan(self._g, int(tall_tiles)))

    def ppo_update(self, lagrangians, rescalings, batch_size, repeat, perms=None, seed=0):
        """k x Engine.ppo_update.  lagrangians: [k][n_critics - 1]; rescalings: [k]; perms: None or per member a list /
        array [repeat][N_i].  -> (list of stats arrays [steps_i, 11], list of stopped passes (-1 = none))."""
        k = len(self.engines)
        lag = np.ascontiguousarray(lagrangians, np.float64).reshape(k, -1)
        resc = np.ascontiguousarray(rescalings, np.float64).reshape(k)
        sizes = [len(e) for e in self.engines]
        cap = max(1, max(-(-n // max(batch_size, 1)) for n in sizes)) * max(repeat, 1)
        stats = [np.empty((cap, _lib.PPO_NSTATS), np.float32) for _ in range(k)]
        sp = (_f32p * k)(*[_ptr(s, _f32p) for s in stats])
        pp, keep = None, []
        if perms is not None:
            for i in range(k):
                a = np.ascontiguousarray(np.stack([np.asarray(p, np.int64) for p in perms[i]]), np.int64)
                assert a.shape == (repeat, sizes[i]), "perms[i] must be [repeat][N_i]"
                keep.append(a)
            pp = (_i64p * k)(*[_ptr(a, _i64p) for a in keep])
        nst = np.zeros(k, np.int64)
        stop = np.zeros(k, np.int32)
        _lib.check(self.lib.fsrl_group_ppo_update(self._g, _ptr(lag, _f64p) if lag.size else None, _ptr(resc, _f64p),
                                                  int(batch_size), int(repeat), pp, int(seed), sp, cap, _ptr(nst, _i64p),
                                                  _ptr(stop, _i32p)))
        for e, n in zip(self.engines, sizes):
            e._n = n
        return [s[:int(n)] for s, n in zip(stats, nst)], [int(x) for x in stop]

    def ppo_update_each(self, lagrangians, rescalings, batch_sizes, repeats, perms=None, seed=0):
        """ppo_update with member i's own minibatch size batch_sizes[i] and number of passes repeats[i] (a sweep; 0 passes: the
        member sits the update out).  perms: None or per member a list / array [repeats[i]][N_i].  Returns what ppo_update returns."""
        k = len(self.engines)
        lag = np.ascontiguousarray(lagrangians, np.float64).reshape(k, -1)
        resc = np.ascontiguousarray(rescalings, np.float64).reshape(k)
        bs = np.ascontiguousarray(batch_sizes, np.int32).reshape(k)
        rp = np.ascontiguousarray(repeats, np.int32).reshape(k)
        sizes = [len(e) for e in self.engines]
        caps = np.array([max(1, -(-n // max(int(b), 1))) * max(int(r), 1) for n, b, r in zip(sizes, bs, rp)], np.int64)
        stats = [np.empty((int(c), _lib.PPO_NSTATS), np.float32) for c in caps]
        sp = (_f32p * k)(*[_ptr(s, _f32p) for s in stats])
        pp, keep = None, []
        if perms is not None:
            for i in range(k):
                a = np.ascontiguousarray([np.asarray(p, np.int64) for p in perms[i]], np.int64).reshape(len(perms[i]), sizes[i])
                assert a.shape == (int(rp[i]), sizes[i]), "perms[i] must be [repeats[i]][N_i]"
                keep.append(a)
            pp = (_i64p * k)(*[_ptr(a, _i64p) for a in keep])
        nst = np.zeros(k, np.int64)
        stop = np.zeros(k, np.int32)
        _lib.check(self.lib.fsrl_group_ppo_update_each(self._g, _ptr(lag, _f64p) if lag.size else None, _ptr(resc, _f64p),
                                                       _ptr(bs, _i32p), _ptr(rp, _i32p), pp, int(seed), sp, _ptr(caps, _i64p),
                                                       _ptr(nst, _i64p), _ptr(stop, _i32p)))
        for e, n in zip(self.engines, sizes):
            e._n = n
        return [s[:int(n)] for s, n in zip(stats, nst)], [int(x) for x in stop]

    def focops_update(self, nus, nu_losses, batch_size, repeat, perms=None, seed=0):
        """k x Engine.focops_update (a group of FOCOPS engines): member i's nu / nu_loss set, then ONE grouped update.
        -> (list of stats arrays [steps_i, 8] as Engine.focops_update, list of stopped passes (-1 = none))."""
        k = len(self.engines)
        assert len(nus) == k and len(nu_losses) == k, "one nu and one nu_loss per member"
        for e, nu, nl in zip(self.engines, nus, nu_losses):
            if e._ctx:                                   # a closed member: the grouped call below reports the destroyed member
                _lib.check(self.lib.fsrl_focops_set_nu(e._ctx, float(nu), float(nl)))
        stats, stopped = self.ppo_update(np.zeros((k, 1)), np.ones(k), batch_size, repeat, perms=perms, seed=seed)
        return [s[:, :_lib.FOCOPS_NSTATS] for s in stats], stopped


class EngineSacGroup(_NativeGroup):
    """k SAC-Lagrangian engines (sac_init, stochastic actor), or k DDPG-Lagrangian engines (sac_init(deterministic=True)),
    of one shape on one GPU, updated in lock step (fsrl_sac_group_*): every launch of an update carries all members that
    still have updates to run.  The group's kind is its first member's; the two kinds do not mix.  Members keep their
    own streams, stores, parameters, Philox keys and statistics rings, and stay ordinary engines between updates (push,
    collect_step with the resident actor, sac_get_params, sac_drain ...).
    The members are all fused (two hidden layers of at most 256 units) or all layered contexts of one `hidden_sizes` and
    `force_layered`: a layered group runs the layered update's launch sequence with every member in each launch, and a member's
    grouped update is then bit-identical to its own sac_update at every group size.
    Prioritised replay (per_enable) is on for every member or for none, switched on BEFORE the group is made; alpha, beta and
    weight_norm may differ.  A grouped update of prioritised members draws each member's batch from its own sum tree and writes its
    new priorities back inside the shared launches; per_state / per_last_weights / per_last_td / sac_last_sample then answer for
    the member's last update of the call."""
    _symbols = "fsrl_sac_group"

    def update(self, batch_size, n_updates, lagrangians=None, rescalings=None):
        """n_updates[i] x Engine.sac_update(batch_size, ..., sync=False) on member i (library RNG), all in lock step.
        lagrangians: None (use_lagrangian off) or [k][n_critics - 1]; rescalings: [k] (default 1).  Enqueues only: the
        statistics rows wait in each member's ring for its sac_drain()."""
        k = len(self.engines)
        n = np.ascontiguousarray(n_updates, np.int32).reshape(k)
        resc = np.ascontiguousarray(np.ones(k) if rescalings is None else rescalings, np.float64).reshape(k)
        lag = None if lagrangians is None else np.ascontiguousarray(lagrangians, np.float64).reshape(k, -1)
        _lib.check(self.lib.fsrl_sac_group_update(self._g, int(batch_size), _ptr(n, _i32p),
                                                  _ptr(lag, _f64p) if lag is not None and lag.size else None, _ptr(resc, _f64p)))


class EngineCvpoGroup(_NativeGroup):
    """k CVPO engines (cvpo_init) of one launch structure on one GPU, updated in lock step (fsrl_cvpo_group_*): every launch of
    an update carries all members that still have updates to run.  Members keep their own streams, stores, parameters, duals,
    Philox keys and statistics rings, and stay ordinary engines between updates (push, collect_step with the resident actor,
    cvpo_pre_update / cvpo_post_update / cvpo_set_thres, own cvpo_update calls, sac_drain ...).
    The members are all fused (two hidden layers of at most 256 units) or all layered contexts of one `hidden_sizes` and
    `force_layered`: a layered group runs the layered update's launch sequence with every member in each launch -- without the
    second actor forward of an M iteration, which recomputes the first: 6 L + 15 + mstep_iter_num (2 L + 6) launches per update
    for L hidden layers -- and a member's grouped update is then bit-identical to its own cvpo_update at every group size."""
    _symbols = "fsrl_cvpo_group"

    def update(self, batch_size, n_updates):
        """n_updates[i] x Engine.cvpo_update(batch_size, sync=False) on member i (library RNG), all in lock step.  Enqueues only:
        the statistics rows wait in each member's ring for its sac_drain()."""
        k = len(self.engines)
        n = np.ascontiguousarray(n_updates, np.int32).reshape(k)
        _lib.check(self.lib.fsrl_cvpo_group_update(self._g, int(batch_size), _ptr(n, _i32p)))


class EngineCollectGroup(_LockStepCollect):
    """k replay-agent engines (all SAC-Lag, all DDPG-Lag or all CVPO: sac_init / cvpo_init) of one network shape on one GPU that
    COLLECT in lock step (fsrl_collect_group_*): one library call and one request to one resident actor kernel per vector step
    for all members, per member bit-identical to its own collect_step.  Independent of the update groups: the members may also
    be in an EngineSacGroup / EngineCvpoGroup, and stay ordinary engines.  EngineGroup's collect interface, so
    GroupCollector(engine_collect_group, collectors) drives it.
    The members (of any of the three kinds) may all be layered contexts of one `hidden_sizes`: the group then has no
    resident kernel -- a request is one launch sequence (L + 2 launches) for all members, actor_set_resident is accepted and has no
    effect, actor_release does nothing and actor_resident_stats counts the requests.
    A fourth kind of member is the on-policy engine that keeps its own streams: CPO and TRPO-Lag engines (which may share a group:
    only the actor matters here), PPO-Lag or FOCOPS engines outside an EngineGroup -- fused or layered, never mixed with replay
    engines.  Their updates stay their own (tr_begin / cpo_learn / trpo_learn) and may run on one host thread per member at once
    (fsrl_amd.policy.TrustPolicyGroup); a member's call that runs during a collect_step of its group is a caller error."""
    _symbols = "fsrl_collect_group"
    _collect_step_symbol = "fsrl_collect_group_step"
    _collect_episodes_symbol = "fsrl_collect_episodes_group"
