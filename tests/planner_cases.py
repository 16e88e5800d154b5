"""The cases of the planner's tests (include/trex_planner.h): the smallest shapes at which its kernels can go wrong, their inputs -
nominal, noise, rewards, done flags, terminal values, strides - and the tolerances, each derived from the reference's own f32 run
(tests/planner_ref.py), the sensor model's rule (tests/sensing_cases.py).

What the shapes exercise: K = 1, 2, 63, 64, 65, 257, 1025 - below, at and above a wavefront, a workgroup's 256 lanes and its
fourfold, so the group kernel's strided loops and tree and the sample launch's last, partial tile -; G = 1 and 3; P = 1, 2, 5
against S = 1, 2, 7, 12, P == S included; A = 1, 4, 25, 50: one Philox block, a whole one, a partial last one, and P A = 250 > 64
(four knot-sum workgroups per group); the three kinds; env_offset up to the last one that fits 32 bits.

Compared bitwise with the reference: sample 0 of every group, the knots of zero-sigma actions, `it`, the action block as the
interpolation of the device's own knots, the returns, best, the temperature-0 nominal, the shifted nominal, the action, exact-zero
weights. Within a tolerance: the Gaussian knots (4 x the largest deviation of the f32 run's knots from the f64 run's), and the
weights, the weighted nominal and the effective sample size, computed from the DEVICE's knots and returns (4 x the same kind of
bound + 2 ulp of the largest operand). Nothing is left out of a comparison.
numpy only. A helper, not a conftest."""
import collections

import numpy as np

import planner_ref as ref

Case = collections.namedtuple("Case", "name G K S P A kind env_offset seed temperature gamma terminal step_pad env_stride flags")
CASES = [
    Case("one", 1, 1, 1, 1, 1, ref.HOLD, 0, 1, 0.0, 1.0, False, 0, 1, ()),
    Case("pairs", 3, 2, 2, 2, 4, ref.LINEAR, 7, 2, 0.5, 0.9, True, 0, 1, ("equal",)),
    Case("wave-1", 1, 63, 7, 5, 25, ref.CUBIC, 0, 3, 0.3, 1.0, False, 5, 3, ()),
    Case("wave", 3, 64, 12, 5, 50, ref.CUBIC, 2 ** 32 - 192, 4, 0.0, 0.9, True, 0, 77, ("nan_one",)),
    Case("wave+1", 3, 65, 7, 2, 4, ref.LINEAR, 1000, 5, 1.0, 1.0, False, 3, 2, ("nan_group", "underflow")),
    Case("constant", 1, 257, 12, 1, 25, ref.HOLD, 0, 6, 0.2, 0.9, True, 0, 1, ()),
    Case("large", 1, 1025, 7, 5, 4, ref.HOLD, 3, 7, 0.5, 1.0, False, 9, 4, ("underflow",)),
    Case("tie", 3, 65, 12, 5, 1, ref.HOLD, 0, 8, 0.0, 1.0, False, 0, 1, ("equal", "nan_one")),
    Case("cubic-257", 3, 257, 12, 5, 25, ref.CUBIC, 65536, 9, 0.25, 0.9, True, 0, 1, ("nan_group",)),
]
BY_NAME = {c.name: c for c in CASES}


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def noise_of(case):
    """(sigma, lo, hi) [A] f32: every third action without noise, every second one between limits tight enough that both clips act"""
    a = np.arange(case.A)
    sigma = np.where(a % 3 == 1, 0.0, 0.1 + 0.05 * (a % 4)).astype(np.float32)
    lo = np.where(a % 2 == 1, -0.05, -10.0).astype(np.float32)
    hi = np.where(a % 2 == 1, 0.08, 10.0).astype(np.float32)
    return sigma, lo, hi


def nominal_of(case):
    rng = np.random.default_rng(100 + case.seed)
    return rng.uniform(-0.3, 0.3, (case.G, case.P, case.A)).astype(np.float32)


Inputs = collections.namedtuple("Inputs", "block reward done terminal step_stride env_stride reward_offset done_offset")


def inputs_of(case):
    """The reward and done columns [S, N] inside ONE f32 block, as a row block holds them: element (s, e) of the reward at
    s step_stride + e env_stride, of done one float behind it where the env stride leaves room (else in a block of its own half);
    done planted at step 0, mid-horizon and the last step on every seventh env each; the flags' scenarios."""
    rng = np.random.default_rng(200 + case.seed)
    S, N, K = case.S, case.G * case.K, case.K
    reward = rng.uniform(-1, 1, (S, N)).astype(np.float32)
    done = np.zeros((S, N), np.float32)
    e = np.arange(N)
    done[0, e % 7 == 1] = 1
    done[S // 2, e % 7 == 2] = 1
    done[S - 1, e % 7 == 3] = 2          # (any non-zero value is done)
    if "equal" in case.flags:            # group 0: one return for all, no done
        reward[:, :K] = reward[:, :1]
        done[:, :K] = 0
    if "underflow" in case.flags:        # every other env of group 0 lies 1000 temperatures below: expf gives an exact 0
        reward[0, 1:K:2] -= np.float32(1000.0 * max(case.temperature, 1.0))
    if "nan_one" in case.flags:
        reward[0, K // 2] = np.nan
    if "nan_group" in case.flags:
        reward[S - 1, N - K:] = np.nan
        done[:, N - K:] = 0
    env_stride = case.env_stride
    step_stride = N * env_stride + case.step_pad
    width = 2 if env_stride >= 2 else 1
    half = S * step_stride
    block = np.full(half * (1 if width == 2 else 2) + 8, 7.0, np.float32)
    at = (np.arange(S)[:, None] * step_stride + e[None, :] * env_stride)
    block[at] = reward
    done_at = at + 1 if width == 2 else at + half
    block[done_at] = done
    terminal = rng.uniform(-2, 2, N).astype(np.float32) if case.terminal else None
    return Inputs(block, reward, done, terminal, step_stride, env_stride, 0, 1 if width == 2 else half)


def reference(case, f32=False, mistake=None):
    """The whole sequence on the host: sample, returns, update, shift by one step, action at step 0 - every stage fed by the one
    before, in the run's own precision."""
    sigma, lo, hi = noise_of(case)
    nominal = nominal_of(case)
    inp = inputs_of(case)
    table = ref.tap_table(case.kind, case.S, case.P)
    knots = ref.sample_knots(nominal, case.K, sigma, lo, hi, case.seed, case.env_offset, 0, f32, mistake)
    actions = ref.actions_of(knots, table, lo, hi, f32)
    R = ref.returns_of(inp.reward, inp.done, inp.terminal, case.gamma, f32, mistake)
    up = ref.update_of(R, knots, nominal, case.K, case.temperature, f32, mistake)
    shifted = ref.shift_of(up["nominal"].astype(np.float32), case.kind, case.S, 1, f32, mistake)
    action = ref.action_of(shifted.astype(np.float32), table, 0, lo, hi, f32)
    return dict(knots=knots, actions=actions, returns=R, shifted=shifted, action=action, **up)


def gaussian(case):
    """[N, P, A] bool: the knots that carry a Gaussian draw"""
    sigma, _, _ = noise_of(case)
    k = np.arange(case.G * case.K) % case.K
    return np.broadcast_to((k > 0)[:, None, None] & (sigma > 0)[None, None, :], (case.G * case.K, case.P, case.A))


def gaussian_bound(case):
    """the largest deviation of the f32 run's knots from the f64 run's"""
    sigma, lo, hi = noise_of(case)
    k64, k32 = (ref.sample_knots(nominal_of(case), case.K, sigma, lo, hi, case.seed, case.env_offset, 0, f) for f in (False, True))
    return float(np.abs(k32.astype(np.float64) - k64).max())


def update_bounds(case, R, knots, nominal):
    """From the DEVICE's returns, knots and nominal: the f64 and the f32 update (whose best, mean return and one-hot weights are
    exact) and the tolerance of the weights [N], of the weighted nominal
    [G, 1, 1] and of the effective sample size [G] - 4 x the f32 run's largest deviation + 2 ulp of the largest operand."""
    u64 = ref.update_of(R, knots, nominal, case.K, case.temperature, False)
    u32 = ref.update_of(R, knots, nominal, case.K, case.temperature, True)
    dev = lambda key: float(np.abs(u32[key].astype(np.float64) - u64[key]).max())
    bound = dict(weights=dev("weights"), nominal=dev("nominal"), ess=float(np.abs(u32["stats"][:, 2].astype(np.float64) - u64["stats"][:, 2]).max()))
    sw = np.where(u64["sum_w"] > 0, u64["sum_w"], 1.0)
    tol = dict(weights=4 * bound["weights"] + 2 * ulp32(1.0),
               nominal=(4 * bound["nominal"] + 2 * ulp32(np.maximum(u64["operand"], u64["operand"] / sw)))[:, None, None],
               ess=4 * bound["ess"] + 2 * ulp32(np.maximum(u64["stats"][:, 2], sw * sw)))
    return u64, u32, bound, tol
