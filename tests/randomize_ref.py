"""numpy restatement of the episode randomisation (include/trex_randomize.h), written from the header's definition and not from
the kernel: the streams and counters over the Philox4x32-10 of tests/sensing_ref.py, episode and row counts, the draws of an
episode, the push bookkeeping and the command resampling. The arithmetic runs in f64 - the reference proper - or, with f32=True,
with every product and sum rounded to f32 as the header orders them: that run is what the device must give bitwise wherever no
sinf or cosf is involved, and its deviation from the f64 run is what tests/randomize_cases.py derives the push-force bound from.

`mistake` plants ONE deliberate error, for the qualification of the cases (every one must be caught by a case):
    value_every_step     the values of an episode are drawn at every row, the counter carrying k
    push_phase_ignored   off = 0
    push_one_longer      a push lasts duration + 1 steps
    push_survives_done   a first row does not zero push_left
    block_by_mask        block and output are taken from the element's rank within the mask
    command_at_one       the command is resampled at k % interval == 1
    sin_cos_swapped      the force is (m sin, m cos, 0)
    env_offset_dropped   the counter carries e, not env_offset + e
numpy only: no torch, no device. A helper, not a conftest."""
import collections

import numpy as np

from sensing_ref import draw_int, key_of, philox4x32, u_half_open

MASS, FRICTION, KP, KD, MAX_FORCE, PUSH, COMMAND = range(7)
EPISODE_STREAM, PUSH_STREAM, COMMAND_STREAM = 4, 5, 6
MAXTERMS, MAXPUSHES, TL = 16, 4, 32
Term = collections.namedtuple("Term", "kind mask index shared lo hi interval duration probability")
MISTAKES = ("value_every_step", "push_phase_ignored", "push_one_longer", "push_survives_done", "block_by_mask", "command_at_one",
            "sin_cos_swapped", "env_offset_dropped")
# one applied row: values [n, T, 32], push_force [n, P, 3], push_left [n, P], command [n, 3], and what happened in it -
# starts: pushes started, cuts: pushes that a first row ended while they still had steps to act on, resamples: commands drawn at
# a row that is not a first one
Row = collections.namedtuple("Row", "values push_force push_left command starts cuts resamples")


def elements(term, nb, nj):
    """the elements a term covers, ascending: bodies (MASS), joints in observation order (KP, KD, MAX_FORCE), [0] otherwise"""
    if term.kind in (FRICTION, COMMAND):
        return [0]
    if term.kind == PUSH:
        return []
    count = nb if term.kind == MASS else nj
    return [i for i in range(count) if term.mask == 0 or (term.mask >> i) & 1]


class Randomizer:
    """The randomisation state of a batch of n envs and what trex_batch_apply_randomization does at a row."""

    def __init__(self, n, nb, nj, terms, seed=0, env_offset=0, f32=False, mistake=None):
        assert mistake is None or mistake in MISTAKES
        self.n, self.nb, self.nj, self.terms = n, nb, nj, [Term(*t) for t in terms]
        self.key, self.f32, self.mistake = key_of(seed), f32, mistake
        self.env_offset = 0 if mistake == "env_offset_dropped" else int(env_offset)
        self.dt = np.float32 if f32 else np.float64
        self.pushes = [t for t, term in enumerate(self.terms) if term.kind == PUSH]
        T, P = len(self.terms), len(self.pushes)
        self.ep, self.k = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.started = np.zeros(n, bool)
        self.values = np.zeros((n, T, TL), self.dt)
        self.off = np.zeros((n, P), np.int64)
        self.push_left = np.zeros((n, P), np.int64)
        self.push_force = np.zeros((n, P, 3), self.dt)
        self.command = np.zeros((n, 3), self.dt)

    def reset(self, mask=None):
        self.started[np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0] = False

    def _words(self, stream, k, block):
        e = self.env_offset + np.arange(self.n)
        return philox4x32((e, k, (stream << 16) | block, self.ep), self.key)

    def _uniform(self, term, r):
        lo, hi, u = self.dt(np.float32(term.lo)), self.dt(np.float32(term.hi)), u_half_open(r).astype(self.dt)
        v = lo + (hi - lo) * u
        assert v.dtype == self.dt
        return v

    def apply(self, done):
        n = self.n
        first = (np.asarray(done) != 0) | ~self.started
        self.ep += first
        self.k = np.where(first, 0, self.k + 1)
        self.started[:] = True
        k, zero = self.k, np.zeros(n, np.int64)
        starts = cuts = resamples = 0
        every = self.mistake == "value_every_step"
        for t, term in enumerate(self.terms):
            if term.kind in (MASS, FRICTION, KP, KD, MAX_FORCE):
                draw = np.ones(n, bool) if every else first
                for rank, i in enumerate(elements(term, self.nb, self.nj)):
                    src = 0 if term.shared else (rank if self.mistake == "block_by_mask" else i)
                    r = self._words(EPISODE_STREAM, k if every else zero, 8 * t + (src >> 2))
                    self.values[:, t, i] = np.where(draw, self._uniform(term, r[src & 3]), self.values[:, t, i])
            elif term.kind == PUSH:
                p = self.pushes.index(t)
                r = self._words(EPISODE_STREAM, zero, 8 * t)
                off = zero if self.mistake == "push_phase_ignored" else draw_int(r[0], 0, term.interval - 1)
                self.off[:, p] = np.where(first, off, self.off[:, p])
                left = self.push_left[:, p].copy()
                cuts += int((first & (left > 1)).sum())
                dec = np.where(left > 0, left - 1, left)
                left = dec if self.mistake == "push_survives_done" else np.where(first, 0, dec)
                due = (left == 0) & ((k + self.off[:, p]) % term.interval == 0)
                r = self._words(PUSH_STREAM, k, t)
                start = due & (u_half_open(r[0]) < float(np.float32(term.probability)))
                if self.f32:
                    a = np.float32(6.2831855) * u_half_open(r[1]).astype(np.float32)
                else:
                    a = float(np.float32(6.2831855)) * u_half_open(r[1])
                m = self._uniform(term, r[2])
                fx, fy = m * np.cos(a), m * np.sin(a)
                if self.mistake == "sin_cos_swapped":
                    fx, fy = fy, fx
                assert fx.dtype == self.dt
                left = np.where(start, term.duration + (1 if self.mistake == "push_one_longer" else 0), left)
                force = np.stack([fx, fy, np.zeros(n, self.dt)], 1)
                keep = (left > 0) & ~start
                self.push_force[:, p] = np.where(start[:, None], force, np.where(keep[:, None], self.push_force[:, p], 0))
                self.push_left[:, p] = left
                starts += int(start.sum())
            else:
                at = 1 if self.mistake == "command_at_one" else 0
                again = ~first & (term.interval > 0) & (k % max(term.interval, 1) == at % max(term.interval, 1)) & (k > 0)
                r0 = self._words(EPISODE_STREAM, zero, 8 * t)
                r1 = self._words(COMMAND_STREAM, k, t)
                for sel, r in ((first, r0), (again, r1)):
                    v = np.where(u_half_open(r[0]) < float(np.float32(term.probability)), self.dt(0), self._uniform(term, r[1]))
                    self.command[:, term.index] = np.where(sel, v, self.command[:, term.index])
                    self.values[:, t, 0] = np.where(sel, v, self.values[:, t, 0])
                resamples += int(again.sum())
        return Row(self.values.copy(), self.push_force.copy(), self.push_left.copy(), self.command.copy(), starts, cuts, resamples)
