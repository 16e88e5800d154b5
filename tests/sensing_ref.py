"""numpy restatement of the sensor model (include/trex_sensing.h), written from the header's definition and not from the kernel:
Philox4x32-10 in uint64 arithmetic (pinned to Random123's known answers by tests/test_sensing_cases_host.py), the streams and
counters, the uniforms and the Box-Muller pairs, episode and row counts, delays, biases, resolution. The arithmetic runs in f64 -
the reference proper - or, with f32=True, with every product and sum rounded to f32 as the header orders them: the deviation of
that run from the f64 run is what tests/sensing_cases.py derives the Gaussian tolerance from.

`mistake` plants ONE deliberate error, for the qualification of the cases (every one must be caught by a case):
    env_column_swapped   env and block change places in the counter
    bias_every_step      the bias counter carries k
    delay_off_by_one     a sensor reads row k - d - 1
    history_kept         a done row does not restart the history: rows of the old episode are read
    sin_cos_swapped      the pair gives (R sin, R cos)
    block_in_group       block and output are taken from the column's place in its group
numpy only: no torch, no device. A helper, not a conftest."""
import collections

import numpy as np

GAUSSIAN, UNIFORM = 0, 1
WHITE, BIAS, DELAY, ACTION = 0, 1, 2, 3
MAXDELAY, MAXGROUPS = 8, 64
Group = collections.namedtuple("Group", "col0 width noise_kind noise bias quantum delay_min delay_max")
MISTAKES = ("env_column_swapped", "bias_every_step", "delay_off_by_one", "history_kept", "sin_cos_swapped", "block_in_group")

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key, rounds=10):
    """counter: 4 broadcastable integer arrays, key: 2 -> 4 uint64 arrays holding 32-bit words"""
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in np.broadcast_arrays(*counter)]
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key)
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c


def key_of(seed):
    seed = int(seed) & (2 ** 64 - 1)
    return seed & 0xFFFFFFFF, seed >> 32


def u_half_open(r):
    """[0, 1): exact in f32 and f64"""
    return (r >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def u_open_closed(r):
    """(0, 1]"""
    return ((r >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24


def draw_int(r, lo, hi):
    return lo + ((r * np.uint64(hi - lo + 1)) >> np.uint64(32)).astype(np.int64)


def normals(r, f32=False, swapped=False):
    """the four standard normals of a block's outputs r[0..3] (arrays): (r0, r1) -> R cos, R sin; (r2, r3) likewise"""
    out = []
    for p in (0, 2):
        u1, u2 = u_open_closed(r[p]), u_half_open(r[p + 1])
        if f32:
            R = np.sqrt(np.float32(-2.0) * np.log(u1.astype(np.float32)))
            a = np.float32(6.2831855) * u2.astype(np.float32)
            pair = [R * np.cos(a), R * np.sin(a)]
            assert pair[0].dtype == np.float32
        else:
            R = np.sqrt(-2.0 * np.log(u1))
            a = 2.0 * np.pi * u2
            pair = [R * np.cos(a), R * np.sin(a)]
        out += pair[::-1] if swapped else pair
    return out


Applied = collections.namedtuple("Applied", "out y t opmax delayed")


class Sensors:
    """The sensing state of a batch of n envs and what trex_batch_apply_sensing does to a block of rows."""

    def __init__(self, n, obs_dim, tail, groups, seed=0, env_offset=0, f32=False, mistake=None):
        assert mistake is None or mistake in MISTAKES
        self.n, self.D, self.tail, self.groups = n, obs_dim, tail, [Group(*g) for g in groups]
        self.key, self.env_offset, self.f32, self.mistake = key_of(seed), int(env_offset), f32, mistake
        D = obs_dim
        self.grp = np.full(D, -1)
        for g, gr in enumerate(self.groups):
            assert (self.grp[gr.col0:gr.col0 + gr.width] == -1).all() and gr.col0 >= 0 and gr.col0 + gr.width <= D
            self.grp[gr.col0:gr.col0 + gr.width] = g
        pick = lambda f, fill: np.array([fill if g < 0 else f(self.groups[g]) for g in self.grp])
        self.noise = pick(lambda g: np.float32(g.noise), np.float32(0)).astype(np.float64)
        self.bias = pick(lambda g: np.float32(g.bias), np.float32(0)).astype(np.float64)
        self.quantum = pick(lambda g: np.float32(g.quantum), np.float32(0)).astype(np.float64)
        self.inv_quantum = np.array([float(np.float32(1.0 / q)) if q > 0 else 0.0 for q in self.quantum])
        self.kind = pick(lambda g: g.noise_kind, 0)
        cols = np.arange(D)
        col0 = pick(lambda g: g.col0, 0)
        rel = cols - col0 if mistake == "block_in_group" else cols
        self.block, self.lane = rel >> 2, rel & 3
        self.ep = np.zeros(n, np.int64)
        self.k = np.zeros(n, np.int64)
        self.started = np.zeros(n, bool)
        self.marked = np.zeros(n, bool)
        self.delay = np.zeros((n, max(len(self.groups), 1)), np.int64)
        self.log = []                        # the clean observation columns of every applied block
        self.begin = np.zeros(n, np.int64)   # index in the log of the first row of each env's episode

    def reset(self, mask=None):
        self.started[np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0] = False

    def _words(self, stream, k):
        """the Philox outputs of every (env, column): [n, D] uint64, one stream"""
        e = (self.env_offset + np.arange(self.n))[:, None]
        tag = (stream << 16) | self.block[None, :]
        if self.mistake == "env_column_swapped":
            ctr = (self.block[None, :], k[:, None], (stream << 16) | e, self.ep[:, None])
        else:
            ctr = (e, k[:, None], tag, self.ep[:, None])
        r = philox4x32(ctr, self.key)
        return r, np.choose(self.lane[None, :], r)

    def apply(self, rows):
        """rows [n, >= D + tail] f32 -> Applied(out [n, D + tail], y: the value before the resolution, t = y * inv_quantum where a
        resolution is set (nan elsewhere), opmax: the largest operand's magnitude, delayed)"""
        rows = np.asarray(rows, np.float32)
        n, D = self.n, self.D
        clean = rows[:, :D].copy()
        first = (rows[:, D + 1] != 0) | ~self.started
        self.ep += first
        self.k = np.where(first, 0, self.k + 1)
        self.started[:] = True
        t_now = len(self.log)
        self.log.append(clean)
        if self.mistake != "history_kept":
            self.begin[first] = t_now
        e = self.env_offset + np.arange(n)
        for g, gr in enumerate(self.groups):
            r0 = philox4x32((e, 0, (DELAY << 16) | g, self.ep), self.key)[0]
            d = draw_int(r0, gr.delay_min, gr.delay_max) if gr.delay_max > gr.delay_min else np.full(n, gr.delay_min)
            self.delay[:, g] = np.where(first, d, self.delay[:, g])
        d_col = np.where(self.grp[None, :] >= 0, self.delay[:, np.maximum(self.grp, 0)], 0)
        if self.mistake == "delay_off_by_one":
            d_col = d_col + (d_col > 0)
        src = np.maximum(t_now - d_col, self.begin[:, None])
        stack = np.stack(self.log)                                      # [t, n, D]
        delayed = stack[src, np.arange(n)[:, None], np.arange(D)[None, :]]
        dt = np.float32 if self.f32 else np.float64
        r_white, w_white = self._words(WHITE, self.k)
        _, w_bias = self._words(BIAS, self.k if self.mistake == "bias_every_step" else np.zeros(n, np.int64))
        sym = lambda w: (2.0 * u_half_open(w) - 1.0).astype(dt)
        z4 = normals(r_white, self.f32, self.mistake == "sin_cos_swapped")
        z = np.where(self.kind[None, :] == UNIFORM, sym(w_white), np.choose(self.lane[None, :], z4)).astype(dt)
        y = delayed.astype(dt)
        b_term = self.bias.astype(dt)[None, :] * sym(w_bias)
        n_term = self.noise.astype(dt)[None, :] * z
        opmax = np.abs(y).astype(np.float64)
        y = np.where(self.bias[None, :] > 0, y + b_term, y)
        opmax = np.maximum(opmax, np.where(self.bias[None, :] > 0, np.maximum(np.abs(b_term), np.abs(y)), 0))
        y = np.where(self.noise[None, :] > 0, y + n_term, y)
        opmax = np.maximum(opmax, np.where(self.noise[None, :] > 0, np.maximum(np.abs(n_term), np.abs(y)), 0))
        assert y.dtype == dt
        has_q = self.quantum[None, :] > 0
        with np.errstate(invalid="ignore"):
            t = y * self.inv_quantum.astype(dt)[None, :]
            yq = self.quantum.astype(dt)[None, :] * np.rint(t)
        final = np.where(has_q, yq, y)
        final = np.where(self.grp[None, :] >= 0, final, clean.astype(dt))
        out = np.concatenate([final, rows[:, D:D + self.tail].astype(dt)], 1)
        return Applied(out, y.astype(np.float64), np.where(has_q, t, np.nan).astype(np.float64), opmax, delayed)


class ActionDelay:
    """trex_batch_set_action_delay + trex_batch_delay_actions"""

    def __init__(self, n, cols, delay_min, delay_max, seed=0, env_offset=0):
        self.n, self.cols, self.lo, self.hi = n, cols, int(delay_min), int(delay_max)
        self.key, self.env_offset = key_of(seed), int(env_offset)
        self.ep, self.k = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.started = np.zeros(n, bool)
        self.delay = np.zeros(n, np.int64)
        self.log, self.begin = [], np.zeros(n, np.int64)

    def reset(self, mask=None):
        self.started[np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0] = False

    def step(self, actions, done_prev=None):
        actions = np.asarray(actions, np.float32)
        first = ~self.started if done_prev is None else (np.asarray(done_prev) != 0) | ~self.started
        self.ep += first
        self.k = np.where(first, 0, self.k + 1)
        self.started[:] = True
        t_now = len(self.log)
        self.log.append(actions.copy())
        self.begin[first] = t_now
        r0 = philox4x32((self.env_offset + np.arange(self.n), 0, ACTION << 16, self.ep), self.key)[0]
        d = draw_int(r0, self.lo, self.hi) if self.hi > self.lo else np.full(self.n, self.lo)
        self.delay = np.where(first, d, self.delay)
        src = np.maximum(t_now - self.delay, self.begin)
        return np.stack(self.log)[src, np.arange(self.n)]
