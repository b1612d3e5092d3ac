"""The host model of the replay sampler (oracle/sampler.py) on its own: Philox4x32-10 against the Random123 known-answer vectors,
the key and the draw words against the library's source text, the n-step chains against tests/golden/ref_shim.VectorReplayBuffer
at EVERY stored slot of empty / single-row / ragged / wrapped stores, and the quality of the streams the counter layout gives
(fixed seeds; caps, not measurements: |z| <= 4, chi-square <= df + 4 sqrt(2 df))."""
import os
import re
import sys

import numpy as np
import pytest

from helpers import GOLDEN
from oracle import sampler as S

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import ref_shim  # noqa: E402  (the buffer classes only: nothing of the reference is imported)

CSRC = os.path.join(os.path.dirname(GOLDEN), os.pardir, "fsrl_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ a mirror of the device store
class Mirror:
    """The rows pushed into an engine, kept by ref_shim.VectorReplayBuffer (tianshou's index semantics, written independently of
    the library's store): the book (size, write head, slot written last) per sub-buffer, the done flags and the columns by SLOT."""

    def __init__(self, env_num, sub, obs_dim=1, act_dim=1):
        self.E, self.sub, self.Do, self.Da = int(env_num), int(sub), int(obs_dim), int(act_dim)
        self.buf = ref_shim.VectorReplayBuffer(self.E * self.sub, self.E)
        assert self.buf.buffers[0].maxsize == self.sub

    def push(self, ids, obs, act, rew, cost, term, trunc, nxt):
        term, trunc = np.asarray(term, bool), np.asarray(trunc, bool)
        ptr, *_ = self.buf.add({"obs": np.asarray(obs, np.float32), "act": np.asarray(act, np.float32), "rew": np.asarray(rew, np.float64),
                                "terminated": term, "truncated": trunc, "done": term | trunc,
                                "obs_next": np.asarray(nxt, np.float32), "info.cost": np.asarray(cost, np.float64)}, list(ids))
        return ptr

    def push_flags(self, ids, done):
        k = len(ids)
        z = np.zeros((k, 1), np.float32)
        return self.push(ids, z, z, np.zeros(k), np.zeros(k), done, np.zeros(k, bool), z)

    @property
    def sizes(self):
        return np.array([len(b) for b in self.buf.buffers], np.int64)

    @property
    def book(self):
        return np.array([[len(b), b._index, int(b.last_index[0])] for b in self.buf.buffers], np.int64)

    @property
    def done(self):
        if self.buf._meta is None:
            return np.zeros(self.E * self.sub, bool)
        return self.buf._meta["done"].copy()

    def valid(self):
        return np.concatenate([e * self.sub + np.arange(n) for e, n in enumerate(self.sizes)])

    def store(self):
        m = self.buf._meta
        return {"obs": m["obs"], "act": m["act"], "rew": m["rew"], "cost": m["info.cost"], "terminated": m["terminated"],
                "truncated": m["truncated"], "obs_next": m["obs_next"]}

    def shim_chains(self, idx, n_step):
        """chain / end flags / terminal index the way the reference's compute_nstep_returns forms them (base_policy.py:453-512)"""
        chain = [np.asarray(idx, np.int64)]
        for _ in range(n_step - 1):
            chain.append(self.buf.next(chain[-1]))
        chain = np.stack(chain)
        end = self.buf._meta["done"][chain] | np.isin(chain, self.buf.unfinished_index())
        return chain, end, chain[-1]


def fill_flags(mirror, seed, steps_of_env, lag_env=None, lag_every=7):
    """seeded done flags pushed in lock step: env e takes steps_of_env[e] rows; lag_env sits out every lag_every-th step"""
    rng = np.random.default_rng(seed)
    left = np.array(steps_of_env, np.int64)
    t = 0
    while (left > 0).any():
        ids = [e for e in range(mirror.E) if left[e] > 0 and not (e == lag_env and t % lag_every == 0)]
        if ids:
            mirror.push_flags(ids, (rng.random(len(ids)) < 0.08) | (t % 13 == 12))
            left[ids] -= 1
        t += 1


STORES = {       # name: (env_num, sub, rows pushed per env, lagging env)
    "empty_env": (3, 16, [9, 0, 14], None),
    "single_row": (1, 8, [1], None),
    "single_row_each": (3, 8, [1, 1, 1], None),
    "ragged": (4, 32, [7, 19, 1, 12], None),
    "just_full": (2, 16, [16, 15], None),
    "wrapped": (3, 40, [100, 86, 93], 1),              # 2.5 times round, env 1 lags: three different write heads
}


# ------------------------------------------------------------------------------------------------ Philox, key, draw words
KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff, ) * 4, (0xffffffff, ) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10, one by one and as one vectorised call"""
    for ctr, key, want in KAT:
        assert " ".join("%08x" % int(x) for x in S.philox4x32_10(ctr, key)) == want
    out = S.philox4x32_10(np.array([k[0] for k in KAT]), np.array([k[1] for k in KAT]))
    assert [" ".join("%08x" % int(x) for x in row) for row in out] == [k[2] for k in KAT]


def test_key_matches_the_librarys_source():
    """the default key and the seed hash as the library's source text states them (host_sac.inc / host_cvpo.inc)"""
    sac, cvpo = _src("host_sac.inc"), _src("host_cvpo.inc")
    default = re.search(r"uint64_t key = (0x[0-9A-Fa-f]+)ull;", sac)
    assert default and int(default.group(1), 16) == S.DEFAULT_KEY == S.key_of(0)
    for text in (sac, cvpo):
        m = re.search(r"if \(seed\) s->key = seed \* (0x[0-9A-Fa-f]+)ull \+ (0x[0-9A-Fa-f]+)ull;", text)
        assert m and int(m.group(1), 16) == S.KEY_MUL and int(m.group(2), 16) == S.DEFAULT_KEY
    assert S.key_of(1) == (S.KEY_MUL + S.DEFAULT_KEY) % 2**64
    assert S.key_of(2**63 + 5) == ((2**63 + 5) * S.KEY_MUL + S.DEFAULT_KEY) % 2**64          # wraps like uint64_t
    assert len({S.key_of(s) for s in range(1000)}) == 1000


def test_draw_words_are_disjoint():
    """for every act_dim up to the header's maximum and every particle count the library accepts, the draw words of the index,
    noise and particle streams never meet (by enumeration), and each stream uses every one of its words once"""
    max_act = int(re.search(r"#define FSRL_MAX_ACT (\d+)", _src("common.hpp")).group(1))
    max_k = int(re.search(r"sample_act_num <= (\d+)", _src("host_cvpo.inc")).group(1))
    assert max_act >= 16 and max_k >= 64
    for Da in range(1, max_act + 1):
        idx, nz = S.index_draw_words(), S.noise_draw_words(Da)
        assert len(nz) == (Da + 1) // 2 and len(set(nz)) == len(nz) and not set(idx) & set(nz)
        for K in range(1, max_k + 1):
            pk = S.particle_draw_words(Da, K)
            assert len(pk) == K * ((Da + 3) // 4) and len(set(pk)) == len(pk)
            assert not set(pk) & set(nz) and not set(pk) & set(idx)
            assert max(pk) < 2**32


def test_streams_are_functions_of_row_draw_update_and_key():
    """a block depends on nothing but (row, draw, update, key): a larger batch extends a smaller one, a wider action extends a
    narrower one's pairs, more particles extend fewer"""
    key = S.key_of(5)
    i_small, i_big = S.sample_indices(key, 3, 10, [50, 70], 100), S.sample_indices(key, 3, 40, [50, 70], 100)
    assert np.array_equal(i_small, i_big[:10])
    (t4, p4), (t8, p8) = S.noise(key, 3, 16, 4), S.noise(key, 3, 32, 8)
    assert np.array_equal(t4, t8[:16, :4]) and np.array_equal(p4, p8[:16, :4])
    t3, _ = S.noise(key, 3, 16, 3)
    assert np.array_equal(t3, t4[:, :3])
    k2, k5 = S.particles(key, 3, 16, 4, 2), S.particles(key, 3, 16, 4, 5)
    assert np.array_equal(k2, k5[:2])
    assert np.array_equal(S.particles(key, 3, 16, 3, 2), k2[..., :3])
    # update counts beyond 32 bits reach the counter's fourth word
    assert not np.array_equal(S.sample_indices(key, 7, 10, [50, 70], 100), S.sample_indices(key, 7 + 2**32, 10, [50, 70], 100))


def test_indices_walk_the_sub_buffers():
    """(word0 * stored) >> 32 counted through the sub-buffers: stored rows only, empty sub-buffers skipped, the first and the last
    stored row reachable"""
    sizes, sub = [3, 0, 5, 0, 2, 0], 8
    valid = np.concatenate([e * sub + np.arange(n) for e, n in enumerate(sizes)])
    seen = set()
    for u in range(40):
        idx = S.sample_indices(S.key_of(2), u, 64, sizes, sub)
        assert np.isin(idx, valid).all()
        seen |= set(idx.tolist())
    assert seen == set(valid.tolist())
    w0 = S._blocks(S.key_of(2), 0, np.arange(64), 0)[:, 0].astype(object)
    k = np.array([(int(w) * 10) >> 32 for w in w0])
    assert np.array_equal(S.sample_indices(S.key_of(2), 0, 64, sizes, sub), valid[k])


# ------------------------------------------------------------------------------------------------ chains
@pytest.mark.parametrize("n_step", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", sorted(STORES))
def test_chains_equal_the_reference_buffer_at_every_slot(name, n_step):
    E, sub, steps, lag = STORES[name]
    m = Mirror(E, sub)
    fill_flags(m, 17, steps, lag)
    if name == "wrapped":
        assert (m.sizes == sub).all() and len(set(m.book[:, 1])) > 1
    slots = m.valid()                                                  # every stored slot, not a sample of them
    chain, end, term = S.chains(slots, n_step, m.book, m.done, sub)
    want_chain, want_end, want_term = m.shim_chains(slots, n_step)
    assert chain.shape == (n_step, slots.size)
    assert np.array_equal(chain, want_chain) and np.array_equal(end, want_end) and np.array_equal(term, want_term)


def test_chains_after_every_push_of_a_wrapping_store():
    """the book and the flags change with every push: the model follows the reference buffer through 3 rounds of a small ring"""
    E, sub = 2, 6
    m = Mirror(E, sub)
    rng = np.random.default_rng(5)
    for t in range(20):
        ids = [0, 1] if t % 4 else [0]
        m.push_flags(ids, rng.random(len(ids)) < 0.25)
        slots = m.valid()
        got, want = S.chains(slots, 3, m.book, m.done, sub), m.shim_chains(slots, 3)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), t


def test_replay_index_with_heads_is_the_reference_buffer():
    """oracle.sac_lag.ReplayIndex with write heads: next / unfinished_index equal ref_shim's on the wrapped store; without heads
    it is what it was (rows without wrap-around)"""
    from oracle.sac_lag import ReplayIndex
    E, sub, steps, lag = STORES["wrapped"]
    m = Mirror(E, sub)
    fill_flags(m, 17, steps, lag)
    ri = ReplayIndex(None, sub, m.done, heads=m.book)
    slots = m.valid()
    assert np.array_equal(ri.next(slots), m.buf.next(slots))
    assert np.array_equal(np.sort(ri.unfinished_index()), np.sort(m.buf.unfinished_index()))
    E, sub, steps, lag = STORES["ragged"]
    m = Mirror(E, sub)
    fill_flags(m, 17, steps, lag)
    plain, heads = ReplayIndex(m.sizes, sub, m.done), ReplayIndex(None, sub, m.done, heads=m.book)
    slots = m.valid()
    assert np.array_equal(plain.next(slots), m.buf.next(slots)) and np.array_equal(heads.next(slots), m.buf.next(slots))
    assert np.array_equal(plain.unfinished_index(), m.buf.unfinished_index())
    assert np.array_equal(heads.unfinished_index(), m.buf.unfinished_index())


# ------------------------------------------------------------------------------------------------ stream quality
def _z_cross(x, y):
    """mean of the product of two independent N(0, 1) samples has variance 1 / n"""
    x, y = np.ravel(x), np.ravel(y)
    return float((x * y).mean() * np.sqrt(x.size))


def test_stream_quality_of_the_model():
    """seed 11, 12 updates, batch 1024, act_dim 8, 4000 stored rows (4 particles): indices uniform over 40 equal bins of the stored
    rows; the noise's mean, variance and kurtosis; no correlation between target and pi noise, neighbouring dimensions, rows,
    updates, particles, particle and target noise, or neighbouring seeds.  Fixed inputs: every |z| <= 4 and the chi-square
    <= df + 4 sqrt(2 df) are caps the model meets with room (chi-square 28.6 on 39, largest |z| 1.8), not measurements."""
    seed, U, B, Da, K = 11, 12, 1024, 8, 4
    sizes, sub = [1000, 1000, 1000, 1000], 1000
    key, key2 = S.key_of(seed), S.key_of(seed + 1)
    idx = np.concatenate([S.sample_indices(key, u, B, sizes, sub) for u in range(U)])
    bins, df = 40, 39
    cnt = np.bincount(idx * bins // 4000, minlength=bins)              # slot == rank among the stored rows here
    expect = idx.size / bins
    chi2 = float(((cnt - expect)**2 / expect).sum())
    print(f"chi-square {chi2:.1f} on {df}")
    assert chi2 <= df + 4 * np.sqrt(2 * df)
    nz = [S.noise(key, u, B, Da) for u in range(U)]
    et, ep = np.stack([n[0] for n in nz]), np.stack([n[1] for n in nz])            # [U][B][Da]
    pk = np.stack([S.particles(key, u, B, Da, K) for u in range(U)])                # [U][K][B][Da]
    et2 = np.stack([S.noise(key2, u, B, Da)[0] for u in range(U)])
    z = {}
    for name, x in (("target", et), ("pi", ep), ("particles", pk)):
        n = x.size
        z[name + " mean"] = float(x.mean() * np.sqrt(n))
        z[name + " variance"] = float((x.var() - 1) / np.sqrt(2 / n))
        z[name + " kurtosis"] = float(((x**4).mean() - 3) / np.sqrt(96 / n))
    z["target x pi"] = _z_cross(et, ep)
    z["neighbouring dimensions"] = _z_cross(et[..., :-1], et[..., 1:])
    z["neighbouring dimensions (pi)"] = _z_cross(ep[..., :-1], ep[..., 1:])
    z["neighbouring dimensions (particles)"] = _z_cross(pk[..., :-1], pk[..., 1:])
    z["neighbouring rows"] = _z_cross(et[:, :-1], et[:, 1:])
    z["neighbouring updates"] = _z_cross(et[:-1], et[1:])
    z["particle k x k+1"] = _z_cross(pk[:, :-1], pk[:, 1:])
    z["particle x target"] = _z_cross(pk, np.broadcast_to(et[:, None], pk.shape))
    z["particle x pi"] = _z_cross(pk, np.broadcast_to(ep[:, None], pk.shape))
    z["seed s x s+1"] = _z_cross(et, et2)
    # the index word against the noise: the row's uniform, centred and scaled to unit variance
    u01 = (idx.reshape(U, B) % sub + 0.5) / sub
    z["index x target"] = _z_cross(np.broadcast_to(((u01 - 0.5) * np.sqrt(12))[..., None], et.shape), et)
    for k, v in z.items():
        print(f"z {k}: {v:+.2f}")
    assert all(abs(v) <= 4 for v in z.values()), z
    assert np.abs(et).max() < 6 and np.abs(pk).max() < 6
