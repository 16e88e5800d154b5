"""numpy restatement of the planner (include/trex_planner.h), written from the header's definition and not from the kernels: the
tap tables, the noise (Philox4x32-10 and the Box-Muller pairs of tests/sensing_ref.py, stream 8), the interpolated actions, the
returns, the update, the shift and the nominal's action. Every function is stateless - the tests feed it what the device holds -
and runs in f64 - the reference proper - or, with f32=True, with every product and sum rounded to f32 in the header's order: the
deviation of that run from the f64 run is what tests/planner_cases.py derives its tolerances from.

`mistake` plants ONE deliberate error, for the qualification of the cases (every one must be caught by a case):
    noise_on_sample_zero          sample 0 of a group is perturbed like the others
    discount_off_by_one           step s is discounted by g_(s+1)
    done_step_reward_dropped      the reward of the step that is done does not count
    tie_to_last                   best is the LARGEST k at the maximum
    knot_env_swapped_in_counter   env and knot change places in the Philox counter
    shift_not_clamped             the shifted knot reads the spline at t_p + steps, beyond the horizon too
numpy only: no torch, no device. A helper, not a conftest."""
import math

import numpy as np

from sensing_ref import key_of, normals, philox4x32

HOLD, LINEAR, CUBIC = 0, 1, 2
KINDS = {"hold": HOLD, "linear": LINEAR, "cubic": CUBIC}
STREAM = 8
MAXSAMPLES, MAXHORIZON, MAXKNOTS, MAXACT = 4096, 256, 32, 64
MISTAKES = ("noise_on_sample_zero", "discount_off_by_one", "done_step_reward_dropped", "tie_to_last", "knot_env_swapped_in_counter",
            "shift_not_clamped")
F32 = np.float32


def tap(kind, P, num, den):
    """the four taps of the knot coordinate num / den: (indices [4], f32 weights [4])"""
    idx, W = [0, 0, 0, 0], [1.0, 0.0, 0.0, 0.0]
    if P == 1 or den == 0:
        pass
    elif kind == HOLD:
        idx = [min(num // den, P - 1)] * 4
    else:
        j = min(num // den, P - 2)
        t = float(num - j * den) / float(den)
        if kind == LINEAR:
            idx, W = [j, j + 1, j + 1, j + 1], [1.0 - t, t, 0.0, 0.0]
        else:
            idx = [max(j - 1, 0), j, j + 1, min(j + 2, P - 1)]
            t2 = t * t
            t3 = t2 * t
            W = [(-t3 + 2.0 * t2 - t) / 2.0, (3.0 * t3 - 5.0 * t2 + 2.0) / 2.0, (-3.0 * t3 + 4.0 * t2 + t) / 2.0, (t3 - t2) / 2.0]
    last = max([c for c in range(4) if W[c] != 0.0] or [0])
    w, total = [F32(0)] * 4, F32(0)
    for c in range(last):
        w[c] = F32(W[c])
        total = F32(total + w[c])
    w[last] = F32(F32(1) - total)
    return idx, w


def tap_table(kind, S, P):
    """the interpolation table: indices [S, 4] and f32 weights [S, 4], one tap set per step"""
    taps = [tap(kind, P, s * (P - 1), S - 1) for s in range(S)]
    return np.array([t[0] for t in taps], np.int64), np.array([t[1] for t in taps], F32)


def shift_table(kind, S, P, steps, mistake=None):
    """the shift table: one tap set per NEW knot"""
    k, end = min(steps, S - 1), (P - 1) * (S - 1)
    taps = []
    for p in range(P):
        num = p * (S - 1) + k * (P - 1)
        taps.append(tap(kind, P, num if mistake == "shift_not_clamped" else min(num, end), S - 1))
    return np.array([t[0] for t in taps], np.int64), np.array([t[1] for t in taps], F32)


def discount(S, gamma):
    """g_s = (float)pow((double)gamma, s), s = 0 .. S"""
    g = float(F32(gamma))
    return np.array([F32(math.pow(g, s)) for s in range(S + 1)], F32)


def clip(v, lo, hi):
    """lo where v < lo, else hi where v > hi, else v (a NaN passes)"""
    with np.errstate(invalid="ignore"):
        return np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(v.dtype)


def taps4(knots, idx, w, dt):
    """knots [..., P, A], one tap set (idx [4], w [4]) -> [..., A]: ((w0 k0 + w1 k1) + w2 k2) + w3 k3 in `dt`"""
    k = knots.astype(dt)
    v = dt(w[0]) * k[..., idx[0], :]
    for c in (1, 2, 3):
        v = v + dt(w[c]) * k[..., idx[c], :]
    assert v.dtype == dt
    return v


def draws(G, K, P, A, seed, env_offset, it, f32=False, mistake=None):
    """z [N, P, A]: the standard normal of every (env, knot, action) - sample 0's too, which the header never uses"""
    N = G * K
    e = (int(env_offset) + np.arange(N))[:, None, None]
    p = np.arange(P)[None, :, None]
    a4 = np.arange((A + 3) // 4)[None, None, :]
    tag = (STREAM << 16) | a4
    ctr = (p, it, tag, e) if mistake == "knot_env_swapped_in_counter" else (e, it, tag, p)
    z4 = normals(philox4x32(ctr, key_of(seed)), f32)                       # four arrays [N, P, A4]
    return np.stack(z4, -1).reshape(N, P, -1)[:, :, :A]


def sample_knots(nominal, K, sigma, lo, hi, seed, env_offset, it, f32=False, mistake=None):
    """nominal [G, P, A] f32 -> the samples' knots [N, P, A] in the run's dtype"""
    dt = F32 if f32 else np.float64
    G, P, A = nominal.shape
    sigma, lo, hi = (np.asarray(x, F32) for x in (sigma, lo, hi))
    z = draws(G, K, P, A, seed, env_offset, it, f32, mistake).astype(dt)
    nom = np.repeat(np.asarray(nominal, F32).astype(dt), K, axis=0)         # [N, P, A]
    noisy = nom + sigma.astype(dt)[None, None, :] * z
    k = (np.arange(G * K) % K)[:, None, None]
    perturbed = (sigma[None, None, :] > 0) & ((k > 0) | (mistake == "noise_on_sample_zero"))
    y = np.where(perturbed, noisy, nom)
    assert y.dtype == dt
    return clip(y, lo.astype(dt), hi.astype(dt))


def actions_of(knots, table, lo, hi, f32=False):
    """knots [N, P, A] -> the action block [S, N, A]: every step's taps, clipped"""
    dt = F32 if f32 else np.float64
    idx, w = table
    lo, hi = np.asarray(lo, F32).astype(dt), np.asarray(hi, F32).astype(dt)
    return np.stack([clip(taps4(knots, idx[s], w[s], dt), lo, hi) for s in range(len(idx))])


def action_of(nominal, table, step, lo, hi, f32=False):
    """trex_planner_action: [G, A]"""
    dt = F32 if f32 else np.float64
    lo, hi = np.asarray(lo, F32).astype(dt), np.asarray(hi, F32).astype(dt)
    idx, w = table
    return clip(taps4(clip(np.asarray(nominal, F32).astype(dt), lo, hi), idx[step], w[step], dt), lo, hi)


def shift_of(nominal, kind, S, steps, f32=False, mistake=None):
    """trex_planner_shift: the new nominal [G, P, A], unclipped"""
    dt = F32 if f32 else np.float64
    P = nominal.shape[1]
    idx, w = shift_table(kind, S, P, steps, mistake)
    return np.stack([taps4(np.asarray(nominal, F32), idx[p], w[p], dt) for p in range(P)], 1)


def returns_of(reward, done, terminal, gamma, f32=False, mistake=None):
    """reward [S, N], done [S, N] or None, terminal [N] or None -> R [N], a return that is not finite as -inf"""
    dt = F32 if f32 else np.float64
    S, N = reward.shape
    g = discount(S, gamma).astype(dt)
    R, live = np.zeros(N, dt), np.ones(N, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            ends = np.zeros(N, bool) if done is None else np.asarray(done[s]) != 0
            gs = g[s + 1] if mistake == "discount_off_by_one" else g[s]
            counts = live & ~ends if mistake == "done_step_reward_dropped" else live
            R = np.where(counts, R + gs * np.asarray(reward[s], F32).astype(dt), R)
            live = live & ~ends
        if terminal is not None:
            R = np.where(live, R + g[S] * np.asarray(terminal, F32).astype(dt), R)
    assert R.dtype == dt
    return np.where(np.isfinite(R), R, -np.inf).astype(dt)


def update_of(R, knots, nominal, K, temperature, f32=False, mistake=None):
    """R [N] (as returns_of leaves them), knots [N, P, A], nominal [G, P, A] -> dict(best [G], weights [N], nominal [G, P, A],
    stats [G, 4], operand [G]: the largest |w_k knot| and partial sum of the weighted knot sums, for a tolerance in ulps)"""
    dt = F32 if f32 else np.float64
    G = len(R) // K
    R = np.asarray(R).astype(dt).reshape(G, K)
    kn = np.asarray(knots).astype(dt).reshape((G, K) + tuple(knots.shape[1:]))
    new = np.asarray(nominal, F32).astype(dt).copy()
    T = dt(F32(temperature))
    R_max = R.max(1)
    at_max = R == R_max[:, None]
    first, lastk = at_max.argmax(1), K - 1 - at_max[:, ::-1].argmax(1)
    none = ~np.isfinite(R_max)
    best = np.where(none, -1, lastk if mistake == "tie_to_last" else first)
    if T > 0:
        with np.errstate(invalid="ignore", under="ignore"):
            w = np.exp((R - R_max[:, None]) / T)
        w = np.where(none[:, None] | np.isneginf(R), 0, w).astype(dt)
    else:
        w = (np.arange(K)[None, :] == best[:, None]).astype(dt)
    assert w.dtype == dt
    sw, sw2, sr, count = np.zeros(G, dt), np.zeros(G, dt), np.zeros(G, dt), np.zeros(G, np.int64)
    acc, operand = np.zeros_like(new), np.zeros(G)
    for k in range(K):
        sw = sw + w[:, k]
        sw2 = sw2 + w[:, k] * w[:, k]
        fin = np.isfinite(R[:, k])
        sr = np.where(fin, sr + np.where(fin, R[:, k], 0), sr)
        count += fin
        term = w[:, k, None, None] * kn[:, k]
        acc = acc + term
        operand = np.maximum(operand, np.maximum(np.abs(term), np.abs(acc)).reshape(G, -1).max(1))
    assert acc.dtype == dt and sw.dtype == dt
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(count > 0, sr / np.maximum(count, 1).astype(dt), 0)
        ess = np.where(sw2 > 0, sw * sw / np.where(sw2 > 0, sw2, 1), 0)
        weighted = acc / np.where(sw > 0, sw, 1)[:, None, None]
    for g in range(G):
        if best[g] >= 0:
            new[g] = kn[g, best[g]] if not T > 0 else weighted[g]
    stats = np.stack([R_max, mean, ess, R[:, 0]], 1).astype(dt)
    return dict(best=best.astype(np.int32), weights=w.reshape(-1), nominal=new, stats=stats, operand=operand, sum_w=sw)
