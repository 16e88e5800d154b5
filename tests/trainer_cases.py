"""Case tables and a deterministic generator for the trainer-side kernels (include/trex_policy.h) at the shapes their padding,
clamping and multi-trip loops can get wrong. numpy only: tests/test_trainer_cases_host.py checks every case on the CPU against
oracle/ppo_oracle.py, tests/test_gpu_trainer_edges.py feeds the same arrays to the kernels. A helper, not a conftest.

Everything is drawn in f64 and rounded to f32-representable values, so that the kernels and the f64 oracle see the SAME numbers.

Conditioning of the learner cases. max() and clip() have branches, and an f32 evaluation may take the other side of one where
the f64 oracle sits on the edge. A case is only a fair reference if no sample sits there, so the generator moves the offending
samples away (never drops them). By the oracle alone, with c = cliprange and m = MARGIN = 1e-3 (the f32 error of the kernel's
log-probability is about 1e-5: the margin is a condition on the inputs, not a tolerance):
  * |ratio - (1 +- c)| >= m;                                   (which side of the surrogate clip)
  * |(v - value_old) -+ c| >= m;                               (which side of the value clip)
  * where the value clip is ACTIVE (|v - value_old| > c): |e1 - e2| >= m max(e1, e2);          (which branch of the value max)
  * where the surrogate clip is ACTIVE (ratio outside [1 - c, 1 + c]): |l1 - l2| >= m max(|l1|, |l2|), unless both are 0.
Where a clip is inactive its two branches are the same function of the parameters (e1 == e2, l1 == l2 exactly in f64), so
either side of the max() gives the same loss and gradient and nothing is required there. Offenders are nudged by NUDGE = 0.01:
logp_old for the ratio conditions, value_old for the value-clip edge, ret for e1 ~ e2; then everything is checked again.
"""
import math

import numpy as np

from oracle import ppo_oracle as P

HID = 64
CLIPRANGE, VF_COEF, CLIP_OBS = 0.2, 0.5, 10.0
LR, ADAM_EPS, MAX_GRAD_NORM = 3e-4, 1e-5, 0.5
MARGIN, NUDGE = 1e-3, 0.01

PARAM_NAMES = ["pi.W1", "pi.b1", "pi.W2", "pi.b2", "pi.W3", "pi.b3", "vf.W1", "vf.b1", "vf.W2", "vf.b2", "vf.W3", "vf.b3", "logstd"]

# ---------------------------------------------------------------- case tables
# act: (D, A, n); row_stride cycles over D, D + 2, D + 5
ACT_CASES = [(1, 1, 1), (7, 1, 31), (8, 16, 32), (9, 17, 33), (75, 25, 65), (96, 32, 64), (97, 31, 95), (121, 32, 33), (126, 32, 97)]
ACT_STRIDE_EXTRA = (0, 2, 5)
ACT_TANH_CASES = ("series", "saturated")       # both at (75, 25, 33)
# observe: (n, D, row_stride - D)
OBSERVE_CASES = [(1, 1, 2), (63, 75, 6), (64, 126, 2), (65, 1, 6), (2049, 126, 6), (4096, 75, 2)]
OBSERVE_DONE_PATTERNS = ("none", "all", "random20", "last")
# GAE
GAE_SHAPES = [(1, 1), (1, 257), (2, 255), (32, 256), (5, 1025)]
GAE_DONE_PATTERNS = ("zero", "one", "first", "last")
GAE_GAMMA_LAM = [(0.99, 0.95), (1.0, 1.0), (0.99, 0.0)]
# Adam: (D, A) whose parameter counts are used
ADAM_DIMS = [(1, 1), (75, 25), (126, 32)]
ADAM_STEPS = 30
# advantage statistics: mb x number of minibatches
STATS_MB = [1, 63, 1023, 1025, 4096]
STATS_NMB = [1, 3]
# learner
LEARN_DIMS = [(1, 1), (8, 16), (9, 17), (31, 31), (32, 32), (33, 1), (64, 25), (65, 32), (95, 17), (96, 32)]      # mb = 70, first = 7
LEARN_MBS = [(1, 0), (31, 5), (32, 0), (33, 5), (2048, 0), (2049, 5), (4096, 5)]                                # (mb, first) at D = 75, A = 25
LEARN_REUSE_MBS = [33, 4096, 33, 1000]


def learn_specs():
    """name -> dict(D, A, mb, first, ent_coef, seed): every learner case of the GPU suite"""
    out = {}
    for i, (D, A) in enumerate(LEARN_DIMS):
        out["dims_D%d_A%d" % (D, A)] = dict(D=D, A=A, mb=70, first=7, ent_coef=0.01, seed=100 + i)
    for i, (mb, first) in enumerate(LEARN_MBS):
        out["mb%d_first%d" % (mb, first)] = dict(D=75, A=25, mb=mb, first=first, ent_coef=0.0, seed=200 + i)
    for i, mb in enumerate(LEARN_REUSE_MBS):
        if i != 2:       # the second mb = 33 call repeats the first one's inputs
            out["reuse_mb%d" % mb] = dict(D=75, A=25, mb=mb, first=3, ent_coef=0.0, seed=300 + i)
    out["split64"] = dict(D=75, A=25, mb=64, first=0, ent_coef=0.01, seed=400)
    return out


# ---------------------------------------------------------------- layout, packing
def layout_rule(D, A):
    """include/trex_policy.h restated: the 13 blocks in order, each starting on a multiple of 4 floats -> (layout, count)"""
    shapes = [(D, HID), (HID,), (HID, HID), (HID,), (HID, A), (A,), (D, HID), (HID,), (HID, HID), (HID,), (HID, 1), (1,), (A,)]
    lay, o = {}, 0
    for name, sh in zip(PARAM_NAMES, shapes):
        lay[name] = (o, sh)
        o = (o + math.prod(sh) + 3) & ~3
    return lay, o


def _oracle_key(name):
    if name == "logstd":
        return "logstd", False
    net, what = name.split(".")
    k = {"1": 0, "2": 2, "3": 4}[what[1]]
    return "%s.%d.%s" % (net, k, "weight" if what[0] == "W" else "bias"), what[0] == "W"


def _theta_to_params(kern, theta):
    """flat [in, out] vector -> the oracle's dict in nn.Sequential naming with [out, in] weights"""
    th = theta.detach().cpu().double().numpy() if hasattr(theta, "detach") else np.asarray(theta, np.float64)
    out = {}
    for name, (off, shape) in kern.layout.items():
        v = th[off:off + math.prod(shape)].reshape(shape)
        if name == "logstd":
            out["logstd"] = v
            continue
        net, what = name.split(".")
        k = {"1": 0, "2": 2, "3": 4}[what[1]]
        out["%s.%d.%s" % (net, k, "weight" if what[0] == "W" else "bias")] = v.T.copy() if what[0] == "W" else v
    return out


def _grads_to_flat(kern, grads):
    flat = np.zeros(kern.param_count)
    for name, (off, shape) in kern.layout.items():
        if name == "logstd":
            g = grads["logstd"]
        else:
            net, what = name.split(".")
            k = {"1": 0, "2": 2, "3": 4}[what[1]]
            g = grads["%s.%d.%s" % (net, k, "weight" if what[0] == "W" else "bias")]
            g = g.T if what[0] == "W" else g
        flat[off:off + math.prod(shape)] = np.asarray(g).reshape(-1)
    return flat


def _params_to_theta(layout, param_count, params):
    """the inverse of _theta_to_params: the oracle's dict -> flat f32 vector (weights [in, out]; pad elements 0)"""
    theta = np.zeros(param_count, np.float32)
    for name, (off, shape) in layout.items():
        key, is_w = _oracle_key(name)
        v = np.asarray(params[key], np.float64)
        v = v.T if is_w else v
        assert tuple(v.shape) == tuple(shape), (name, v.shape, shape)
        theta[off:off + math.prod(shape)] = v.reshape(-1)
    return theta


# ---------------------------------------------------------------- generators
def f32r(x):
    """round to the nearest f32, keep f64"""
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def make_params(D, A, rng, out_gain=0.3):
    """MlpPolicy-shaped parameters away from any special point: pre-activations of O(1), non-zero biases and logstd"""
    p = {}
    for net, n_out in (("pi", A), ("vf", 1)):
        p[net + ".0.weight"] = rng.standard_normal((HID, D)) / math.sqrt(D)
        p[net + ".0.bias"] = 0.3 * rng.standard_normal(HID)
        p[net + ".2.weight"] = rng.standard_normal((HID, HID)) / math.sqrt(HID)
        p[net + ".2.bias"] = 0.3 * rng.standard_normal(HID)
        p[net + ".4.weight"] = (out_gain if net == "pi" else 1.0) * rng.standard_normal((n_out, HID)) / math.sqrt(HID)
        p[net + ".4.bias"] = 0.2 * rng.standard_normal(n_out)
    p["logstd"] = rng.uniform(-0.7, 0.2, A)
    return {k: f32r(v) for k, v in p.items()}


def preactivations(params, obs):
    """{(net, layer): [n, 64] pre-activations of the two hidden layers}, by the oracle's own matrices"""
    out = {}
    for net in ("pi", "vf"):
        z1 = obs @ params[net + ".0.weight"].T + params[net + ".0.bias"]
        z2 = np.tanh(z1) @ params[net + ".2.weight"].T + params[net + ".2.bias"]
        out[(net, 1)], out[(net, 2)] = z1, z2
    return out


def act_case(D, A, n, index, tanh_mode=None):
    """Inputs of one trex_policy_act call and the oracle's outputs for them."""
    rng = np.random.default_rng(1000 + 17 * index + (0 if tanh_mode is None else 500 + len(tanh_mode)))
    stride = D + ACT_STRIDE_EXTRA[index % 3]
    params = make_params(D, A, rng)
    stats = dict(obs_mean=f32r(rng.uniform(-2, 2, D)), obs_var=f32r(rng.uniform(0.3, 9.0, D)), obs_count=100.0, ret_mean=0.0,
                 ret_var=4.0, ret_count=100.0)
    rows = np.full((n, stride), 777.0)           # the columns behind the observation are never read: anything
    rows[:, :D] = stats["obs_mean"] + np.sqrt(stats["obs_var"]) * rng.standard_normal((n, D)) * rng.uniform(0.2, 2.5, D)
    rows[rng.integers(n), rng.integers(D)] = 1e4     # clips high
    if n * D > 1:
        i, k = rng.integers(n), rng.integers(D)
        rows[i, k] = -1e4 if rows[i, k] != 1e4 else 1e4
    rows = f32r(rows)
    noise = f32r(rng.standard_normal((n, A)))
    obs_n = np.clip((rows[:, :D] - stats["obs_mean"]) / np.sqrt(stats["obs_var"] + 1e-8), -CLIP_OBS, CLIP_OBS)
    if tanh_mode == "series":
        # every hidden pre-activation below 0.1 in magnitude: tanh_fast's series branch
        for layer, keys in ((1, (".0.weight", ".0.bias")), (2, (".2.weight", ".2.bias"))):
            for net in ("pi", "vf"):
                s = 0.08 / np.abs(preactivations(params, obs_n)[(net, layer)]).max()
                for k in keys:
                    params[net + k] = f32r(params[net + k] * s)
    elif tanh_mode == "saturated":
        # most units far in the saturated branch, through their BIASES (a large bias keeps the unit well-conditioned; large
        # weights would amplify the f32 error of the few units that stay near 0): +-25 (exp2 finite), +-60 (exp2 = inf)
        for net in ("pi", "vf"):
            for k in (".0.bias", ".2.bias"):
                b = params[net + k].copy()
                kind = rng.permutation(HID) % 5          # 0, 1: +-25   2, 3: +-60   4: as drawn
                sign = np.where(rng.random(HID) < 0.5, -1.0, 1.0)
                b[kind < 2] = 25.0 * sign[kind < 2]
                b[(kind >= 2) & (kind < 4)] = 60.0 * sign[(kind >= 2) & (kind < 4)]
                params[net + k] = f32r(b)
    mean, logstd, value = P.policy_forward(params, obs_n)
    actions = P.sample_action(mean, logstd, noise)
    return dict(D=D, A=A, n=n, row_stride=stride, params=params, stats=stats, rows=rows, noise=noise, obs_n=obs_n, mean=mean,
                actions=actions, neglogp=P.neglogp(mean, logstd, actions), value=value)


def learn_quantities(case):
    """The oracle's view of a learner case: its loss/gradient call and the per-sample branch quantities derived from it."""
    idx = case["idx"]
    out, grads = P.ppo_loss_and_grads(case["params"], case["obs"][idx], case["act"][idx], -case["logp_old"][idx], case["value_old"][idx],
                                      case["adv"][idx], case["ret"][idx], cliprange=CLIPRANGE, ent_coef=case["ent_coef"], vf_coef=VF_COEF)
    c = CLIPRANGE
    ratio, v, a = out["ratio"], out["value"], out["adv_normalised"]
    v0, R = case["value_old"][idx], case["ret"][idx]
    l1, l2 = -a * ratio, -a * np.clip(ratio, 1 - c, 1 + c)
    vclip = v0 + np.clip(v - v0, -c, c)
    e1, e2 = (v - R) ** 2, (vclip - R) ** 2
    return dict(out=out, grads=grads, ratio=ratio, dv=v - v0, l1=l1, l2=l2, e1=e1, e2=e2,
                pg_clip=(ratio < 1 - c) | (ratio > 1 + c), vf_clip=np.abs(v - v0) > c)


def learn_violations(q):
    """per-sample masks of the four conditioning rules (module docstring); all False = well-conditioned"""
    c, m = CLIPRANGE, MARGIN
    ratio_edge = np.minimum(np.abs(q["ratio"] - (1 - c)), np.abs(q["ratio"] - (1 + c))) < m
    dv_edge = np.minimum(np.abs(q["dv"] - c), np.abs(q["dv"] + c)) < m
    e_tie = q["vf_clip"] & (np.abs(q["e1"] - q["e2"]) < m * np.maximum(q["e1"], q["e2"]))
    l_tie = q["pg_clip"] & (np.abs(q["l1"] - q["l2"]) < m * np.maximum(np.abs(q["l1"]), np.abs(q["l2"])))
    return dict(ratio_edge=ratio_edge, dv_edge=dv_edge, e_tie=e_tie, l_tie=l_tie)


def learn_case(D, A, mb, first, ent_coef, seed):
    """Rollout buffers of N = first + mb + 100 samples, a permutation, and the minibatch perm[first : first + mb] made
    well-conditioned. Returns the inputs, the advantage statistics (f32-rounded, as the kernel takes them) and the oracle's
    loss terms and flat-able gradients."""
    rng = np.random.default_rng(seed)
    N = first + mb + 100
    params = make_params(D, A, rng)
    obs = f32r(np.clip(rng.standard_normal((N, D)) * rng.uniform(0.3, 2.0, D), -CLIP_OBS, CLIP_OBS))
    mean, logstd, v = P.policy_forward(params, obs)
    act = f32r(P.sample_action(mean, logstd, rng.standard_normal((N, A))))
    logp_old = f32r(-P.neglogp(mean, logstd, act) + 0.3 * rng.standard_normal(N))       # an older policy: ratios leave the clip range
    value_old = f32r(v + 0.3 * rng.standard_normal(N))
    ret = f32r(value_old + rng.standard_normal(N))
    adv = f32r(2.0 * rng.standard_normal(N) + 0.5)
    perm = rng.permutation(N).astype(np.int64)
    idx = perm[first:first + mb]
    case = dict(D=D, A=A, mb=mb, first=first, N=N, ent_coef=ent_coef, params=params, obs=obs, act=act, logp_old=logp_old,
                value_old=value_old, ret=ret, adv=adv, perm=perm, idx=idx, nudged=0)
    for _ in range(200):
        q = learn_quantities(case)
        bad = learn_violations(q)
        if not any(b.any() for b in bad.values()):
            break
        r_bad = bad["ratio_edge"] | bad["l_tie"]
        case["logp_old"][idx[r_bad]] = f32r(case["logp_old"][idx[r_bad]] + NUDGE)
        case["value_old"][idx[bad["dv_edge"]]] = f32r(case["value_old"][idx[bad["dv_edge"]]] + NUDGE)
        e_bad = bad["e_tie"] & ~bad["dv_edge"]
        case["ret"][idx[e_bad]] = f32r(case["ret"][idx[e_bad]] + NUDGE)
        case["nudged"] += int(r_bad.sum() + bad["dv_edge"].sum() + e_bad.sum())
    else:
        raise AssertionError("learn_case(%r): still ill-conditioned after 200 rounds of nudging" % ((D, A, mb, first, seed),))
    a = case["adv"][idx]
    case["adv_stats"] = np.array([a.mean(), 1.0 / (a.std() + 1e-8)]).astype(np.float32)
    case["q"] = q
    return case


_LEARN_CACHE = {}


def learn_case_by_name(name):
    """cached: built once per process, shared, never changed by a test"""
    if name not in _LEARN_CACHE:
        _LEARN_CACHE[name] = learn_case(**learn_specs()[name])
    return _LEARN_CACHE[name]


def done_pattern(kind, shape, rng):
    d = np.zeros(shape)
    if kind in ("all", "one"):
        d[...] = 1.0
    elif kind == "random20":
        d[rng.random(shape) < 0.2] = 1.0
    elif kind == "last":          # observe: only the last env; GAE: only t = T - 1
        d[-1] = 1.0
    elif kind == "first":         # GAE: only t = 0
        d[0] = 1.0
    else:
        assert kind in ("none", "zero"), kind
    return d


def observe_sequence(n, D, extra):
    """Row blocks [n, D + extra] of one reset (with_reward = False) and four reward steps with the done patterns of
    OBSERVE_DONE_PATTERNS; observations with a mean and spread that move from step to step."""
    rng = np.random.default_rng(5000 + 131 * n + D)
    steps = []
    for t in range(1 + len(OBSERVE_DONE_PATTERNS)):
        rows = np.full((n, D + extra), -555.0)
        rows[:, :D] = (3.0 + t) + (1.5 + 0.5 * t) * rng.standard_normal((n, D)) * rng.uniform(0.5, 2.0, D)
        rows[:, D] = -100.0 * rng.random(n) - 1.0
        rows[:, D + 1] = done_pattern(OBSERVE_DONE_PATTERNS[t - 1], (n,), rng) if t else 0.0
        steps.append(f32r(rows))
    return steps


def gae_case(T, n, pattern, index):
    rng = np.random.default_rng(7000 + index)
    raw = f32r(-50.0 * rng.random((T, n)))
    scale = f32r(0.02 + 0.01 * rng.random(T))
    scale[rng.integers(T)] = 10.0               # this step's rewards clip
    done = done_pattern(pattern, (T, n), rng)
    val = f32r(rng.standard_normal((T + 1, n)))
    return dict(raw=raw, scale=scale, done=done, val=val)
