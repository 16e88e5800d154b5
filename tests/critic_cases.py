"""Cases of the privileged critic (include/trex_policy_critic.h), built on tests/trainer_cases.py: the policy half of a case comes
from a trainer case at D, the value half from ANOTHER trainer case at Dv - other rows, other moments, other parameters -, so that
nothing the value net reads can be mistaken for what the policy net reads. numpy only: tests/test_critic_ref.py qualifies every
case on the CPU, tests/test_gpu_critic.py feeds the same arrays to the kernels. A helper, not a conftest."""
import numpy as np

import critic_ref as CR
import trainer_cases as tc

# act: (D, Dv, A, n); strides cycle over +0 / +2 / +5 and stride_v != row_stride
ACT_CASES = [(1, 1, 1, 1), (8, 9, 16, 32), (9, 8, 17, 33), (126, 1, 32, 97), (1, 126, 1, 65), (75, 96, 25, 33), (93, 96, 25, 64)]
# critic observe: (n, Dv)
OBSERVE_CASES = [(1, 1), (65, 96), (2049, 126)]
# learner: (D, Dv, A, mb, first)
LEARN_CASES = [(1, 96, 25, 70, 7), (96, 1, 25, 70, 7), (33, 64, 25, 70, 7), (75, 96, 25, 70, 7), (32, 32, 25, 70, 7),
               (75, 96, 25, 33, 7), (75, 96, 25, 2049, 7)]

PI_KEYS = ["pi.0.weight", "pi.0.bias", "pi.2.weight", "pi.2.bias", "pi.4.weight", "pi.4.bias", "logstd"]
VF_KEYS = ["vf.0.weight", "vf.0.bias", "vf.2.weight", "vf.2.bias", "vf.4.weight", "vf.4.bias"]


def _mix(params_pi, params_vf):
    out = {k: params_pi[k] for k in PI_KEYS}
    out.update({k: params_vf[k] for k in VF_KEYS})
    return out


def act_case(D, Dv, A, n, index):
    """the inputs of one trex_policy_critic_act call and the oracle's outputs: `pi` and `vf` are the two trainer cases"""
    pi = tc.act_case(D, A, n, index)
    vf = tc.act_case(Dv, A, n, index + 101)
    stride = pi["row_stride"]
    extra_v = [e for e in tc.ACT_STRIDE_EXTRA[(index + 1) % 3:] + tc.ACT_STRIDE_EXTRA if Dv + e != stride][0]
    stride_v = Dv + extra_v
    rows_v = np.full((n, stride_v), 777.0)
    rows_v[:, :Dv] = vf["rows"][:, :Dv]
    return dict(D=D, Dv=Dv, A=A, n=n, row_stride=stride, stride_v=stride_v, params=_mix(pi["params"], vf["params"]),
                stats=pi["stats"], stats_v=dict(mean=vf["stats"]["obs_mean"], var=vf["stats"]["obs_var"], count=vf["stats"]["obs_count"]),
                rows=pi["rows"], rows_v=rows_v, noise=pi["noise"], obs_n=pi["obs_n"], obs_v_n=vf["obs_n"], actions=pi["actions"],
                neglogp=pi["neglogp"], value=vf["value"], pi=pi, vf=vf)


def learn_quantities(case):
    """critic_ref's view of a learner case, in the form trainer_cases.learn_violations reads"""
    idx, c = case["idx"], tc.CLIPRANGE
    out, grads = CR.loss_and_grads(case["params"], case["obs"][idx], case["obs_v"][idx], case["act"][idx], -case["logp_old"][idx],
                                   case["value_old"][idx], case["adv"][idx], case["ret"][idx], cliprange=c, ent_coef=case["ent_coef"],
                                   vf_coef=tc.VF_COEF)
    ratio, v, a = out["ratio"], out["value"], out["adv_normalised"]
    v0, R = case["value_old"][idx], case["ret"][idx]
    l1, l2 = -a * ratio, -a * np.clip(ratio, 1 - c, 1 + c)
    vclip = v0 + np.clip(v - v0, -c, c)
    e1, e2 = (v - R) ** 2, (vclip - R) ** 2
    return dict(out=out, grads=grads, ratio=ratio, dv=v - v0, l1=l1, l2=l2, e1=e1, e2=e2,
                pg_clip=(ratio < 1 - c) | (ratio > 1 + c), vf_clip=np.abs(v - v0) > c)


def learn_case(D, Dv, A, mb, first, seed):
    """A learner case whose policy half - parameters, obs, act, logp_old, adv, the permutation - is trainer_cases.learn_case at D
    and whose value half - parameters, obs_v, value_old, ret - is another one at Dv, its samples carried over position by position
    of the minibatch (the other samples in index order). The conditioning of trainer_cases holds half by half: the surrogate's
    rules read the policy half alone, the value loss's rules the value half alone; tests/test_critic_ref.py checks it whole."""
    pi = tc.learn_case(D, A, mb, first, 0.01, seed)
    vf = tc.learn_case(Dv, A, mb, first, 0.01, seed + 50)
    N = pi["N"]
    assert vf["N"] == N
    rest = lambda c: np.setdiff1d(np.arange(N), c["idx"])
    src = np.empty(N, np.int64)               # sample i of the combined case takes its value half from sample src[i] of `vf`
    src[pi["idx"]] = vf["idx"]
    src[rest(pi)] = rest(vf)
    case = dict(D=D, Dv=Dv, A=A, mb=mb, first=first, N=N, ent_coef=0.01, params=_mix(pi["params"], vf["params"]), obs=pi["obs"],
                obs_v=vf["obs"][src], act=pi["act"], logp_old=pi["logp_old"], value_old=vf["value_old"][src], ret=vf["ret"][src],
                adv=pi["adv"], perm=pi["perm"], idx=pi["idx"], adv_stats=pi["adv_stats"], pi=pi, vf=vf)
    case["q"] = learn_quantities(case)
    return case


_LEARN_CACHE = {}


def learn_case_by_index(i):
    """cached: built once per process, shared, never changed by a test"""
    if i not in _LEARN_CACHE:
        D, Dv, A, mb, first = LEARN_CASES[i]
        _LEARN_CACHE[i] = learn_case(D, Dv, A, mb, first, 600 + i)
    return _LEARN_CACHE[i]


def observe_sequence(n, Dv, extra=3):
    """three critic row blocks [n, Dv + extra] whose mean and spread move; the columns behind Dv hold NaN: never read"""
    rng = np.random.default_rng(9000 + 7 * n + Dv)
    steps = []
    for t in range(3):
        rows = np.full((n, Dv + extra), np.nan)
        rows[:, :Dv] = (2.0 - t) + (1.0 + 0.7 * t) * rng.standard_normal((n, Dv)) * rng.uniform(0.5, 2.0, Dv)
        steps.append(np.asarray(rows, np.float32).astype(np.float64))
    return steps
