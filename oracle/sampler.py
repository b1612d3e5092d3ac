"""Exact host model of the replay agents' device-side sampler (library-RNG mode of SAC-Lag, DDPG-Lag, CVPO and their groups).

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  numpy only; written from the definitions, not from the kernels:

  Philox4x32-10          Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3" (SC'11), Random123 `philox.h`
  the n-step index chain tianshou 0.5 ReplayBuffer.next / unfinished_index (restated)
  Box-Muller             n0 = sqrt(-2 ln u1) cos(2 pi u2), n1 = sqrt(-2 ln u1) sin(2 pi u2), in float64

Counter layout ("The replay sampler's streams"): one Philox block per
    counter = (row b, draw word, update count lo, update count hi),   key = (key lo, key hi)
where key = key_of(seed) of the last non-zero seed the context was given (DEFAULT_KEY before any) and the update count is the
number of updates the context has run so far, by either RNG mode.  Draw words:
    0                        word 0 of the block -> the row's index
    1 + d0 / 2               d0 = 0, 2, ...: words 0, 1 -> eps_target[b, d0 : d0 + 2], words 2, 3 -> eps_pi[b, d0 : d0 + 2]
    0x100 + 4 kp + d0 / 4    d0 = 0, 4, ...: words 0 .. 3 -> particle kp's noise [kp, b, d0 : d0 + 4]        (CVPO)
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
MASK64 = (1 << 64) - 1
DEFAULT_KEY = 0x243F6A8885A308D3           # the key of a context that was never seeded
KEY_MUL = 0x9E3779B97F4A7C15
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
DRAW_INDEX, DRAW_NOISE0, DRAW_PARTICLE0 = 0, 1, 0x100


def key_of(seed=0):
    """64-bit Philox key of a context last seeded with `seed`; seed 0 means "never seeded" (a zero seed leaves the key alone)."""
    seed = int(seed)
    return DEFAULT_KEY if seed == 0 else (seed * KEY_MUL + DEFAULT_KEY) & MASK64


def philox4x32_10(counter4, key2):
    """counter4: [..., 4], key2: [..., 2] or (k0, k1) (32-bit words) -> [..., 4] uint64 holding 32-bit words.
    uint64 arithmetic masked to 32 bits: the product of two 32-bit words fits 64 bits, hi = p >> 32, lo = p & M32."""
    c = np.asarray(counter4, np.uint64) & M32
    k = np.broadcast_to(np.asarray(key2, np.uint64) & M32, c.shape[:-1] + (2, ))
    c0, c1, c2, c3 = (c[..., j].copy() for j in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return np.stack([c0, c1, c2, c3], -1)


def _blocks(key, counter, rows, draw):
    """the Philox blocks of rows `rows` at draw word(s) `draw` (broadcast together) -> [..., 4]"""
    key, counter = int(key) & MASK64, int(counter) & MASK64
    rows, draw = np.broadcast_arrays(np.asarray(rows, np.uint64), np.asarray(draw, np.uint64))
    ctr = np.stack([rows, draw, np.full(rows.shape, counter & 0xFFFFFFFF, np.uint64),
                    np.full(rows.shape, counter >> 32, np.uint64)], -1)
    return philox4x32_10(ctr, (key & 0xFFFFFFFF, key >> 32))


def box_muller(a, b):
    """two 32-bit words -> (n0, n1, rad) in float64, from the 24-bit uniforms u1 in (0, 1] and u2 in [0, 1)"""
    u1 = ((np.asarray(a, np.uint64) >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (np.asarray(b, np.uint64) >> np.uint64(8)).astype(np.float64) / 16777216.0
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2), rad


# ---------------------------------------------------------------------------------------------- draw words
def index_draw_words():
    return [DRAW_INDEX]


def noise_draw_words(Da):
    return [DRAW_NOISE0 + d0 // 2 for d0 in range(0, int(Da), 2)]


def particle_draw_words(Da, K):
    return [DRAW_PARTICLE0 + 4 * kp + d0 // 4 for kp in range(int(K)) for d0 in range(0, int(Da), 4)]


# ---------------------------------------------------------------------------------------------- indices and chains
def sample_indices(key, counter, B, sizes, sub_size):
    """B uniform rows of the stored ones: k = (word0 * stored) >> 32 counts through the sub-buffers in order; sizes[e] = rows
    held by sub-buffer e, which owns slots [e * sub_size, (e + 1) * sub_size).  -> int64 [B] slot indices"""
    sizes = np.asarray(sizes, np.int64)
    stored = int(sizes.sum())
    assert stored > 0
    w0 = _blocks(key, counter, np.arange(int(B)), DRAW_INDEX)[:, 0]
    k = ((w0 * np.uint64(stored)) >> np.uint64(32)).astype(np.int64)
    env = np.zeros(int(B), np.int64)
    for e in range(len(sizes) - 1):                    # walk: past sub-buffer e while the count does not fall inside it
        m = (env == e) & (k >= sizes[e])
        k[m] -= sizes[e]
        env[m] += 1
    return env * int(sub_size) + k


def chains(idx, n_step, book, done_flags, sub_size):
    """tianshou's n-step chain of every sampled row.  book[e] = (size, index, last_index) of sub-buffer e: rows held, write
    head, slot written last (all local); done_flags: terminated | truncated per SLOT.
    -> (chain [n_step][B]: chain[0] = idx, chain[n] = next(chain[n - 1]);  end [n_step][B]: done | unfinished tail at
    chain[n];  terminal = chain[-1])"""
    book = np.asarray(book, np.int64).reshape(-1, 3)
    done = np.asarray(done_flags).astype(bool)
    sub = int(sub_size)
    size, head, last = book[:, 0], book[:, 1], book[:, 2]
    # unfinished_index: per sub-buffer the slot before the write head, if it holds a row that does not end an episode
    tail = np.where(size > 0, (head - 1) % np.maximum(size, 1), 0) + np.arange(len(book)) * sub
    unfinished = tail[(size > 0) & ~done[tail]]
    end_flag = done.copy()
    end_flag[unfinished] = True
    cur = np.asarray(idx, np.int64).copy()
    out = [cur]
    for _ in range(int(n_step) - 1):
        env = cur // sub
        local = cur - env * sub
        stop = done[cur] | (local == last[env])
        cur = (local + 1 - stop.astype(np.int64)) % np.maximum(size[env], 1) + env * sub
        out.append(cur)
    chain = np.stack(out)
    return chain, end_flag[chain], chain[-1].copy()


# ---------------------------------------------------------------------------------------------- noise
def noise(key, counter, B, Da, with_rad=False):
    """the two rsample blocks -> (eps_target, eps_pi) float64 [B][Da] (+ the Box-Muller radius of every entry)"""
    B, Da = int(B), int(Da)
    out = np.zeros((2, 2, B, Da + 1))
    for d0 in range(0, Da, 2):
        w = _blocks(key, counter, np.arange(B), DRAW_NOISE0 + d0 // 2)
        for s in range(2):                              # words 0, 1: the target pair; words 2, 3: the pi pair
            n0, n1, rad = box_muller(w[:, 2 * s], w[:, 2 * s + 1])
            out[0, s, :, d0], out[0, s, :, d0 + 1] = n0, n1
            out[1, s, :, d0] = out[1, s, :, d0 + 1] = rad
    out = out[..., :Da]
    return (out[0, 0], out[0, 1], out[1, 0], out[1, 1]) if with_rad else (out[0, 0], out[0, 1])


def particles(key, counter, B, Da, K, with_rad=False):
    """CVPO's K particle blocks -> float64 [K][B][Da] (+ the Box-Muller radius of every entry)"""
    B, Da, K = int(B), int(Da), int(K)
    val, radius = np.zeros((K, B, Da + 3)), np.zeros((K, B, Da + 3))
    kp = np.arange(K)[:, None]
    for d0 in range(0, Da, 4):
        w = _blocks(key, counter, np.arange(B)[None, :], DRAW_PARTICLE0 + 4 * kp + d0 // 4)      # [K][B][4]
        for s in range(2):
            n0, n1, rad = box_muller(w[..., 2 * s], w[..., 2 * s + 1])
            val[..., d0 + 2 * s], val[..., d0 + 2 * s + 1] = n0, n1
            radius[..., d0 + 2 * s] = radius[..., d0 + 2 * s + 1] = rad
    return (val[..., :Da], radius[..., :Da]) if with_rad else val[..., :Da]
