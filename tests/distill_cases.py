"""Cases of policy distillation (include/trex_policy_distill.h), built on tests/trainer_cases.py's generators (make_params,
layout_rule, f32r: imported, that file is not edited). numpy only: tests/test_distill_ref.py runs them on the CPU,
tests/test_gpu_distill.py feeds the same arrays to the kernels. A helper, not a conftest.

Everything is drawn in f64 and rounded to f32-representable values, so that the kernels and the f64 reference see the SAME numbers.
The two losses have no branch in them (no max, no clip), so no sample needs conditioning as the PPO cases do.

A case is a student (MlpPolicy-shaped parameters, logstd in [-0.7, 0.2]), rollout buffers of N = first + mb + 100 samples - the
student's normalised observations, a teacher's mean and value on the same samples (a second parameter draw evaluated on those
observations: the numbers only have to be of the right size and away from the student's) - a teacher logstd in [-2, 0.5], and a
permutation; the minibatch is perm[first : first + mb)."""
import numpy as np

import distill_ref as DR
from oracle import ppo_oracle as P
from trainer_cases import CLIP_OBS, f32r, layout_rule, make_params  # noqa: F401  (layout_rule: re-exported for the tests)

DIMS = [(1, 1), (33, 1), (64, 25), (75, 25), (96, 32)]               # (D, A) at mb = 70, first = 7
MBS = [(1, 0), (31, 5), (32, 0), (33, 5), (2049, 5)]                 # (mb, first) at D = 75, A = 25
KINDS = [("mse", DR.MSE), ("kl", DR.KL)]
VF_COEFS = [0.0, 0.5]
GRAD_SCALES = [1.0, 0.5]


def shapes():
    """name -> (D, A, mb, first, seed): the ten shapes; every one runs both kinds, both vf_coef and both grad_scale"""
    out = {}
    for i, (D, A) in enumerate(DIMS):
        out["dims_D%d_A%d" % (D, A)] = (D, A, 70, 7, 1900 + i)
    for i, (mb, first) in enumerate(MBS):
        out["mb%d_first%d" % (mb, first)] = (75, 25, mb, first, 1950 + i)
    return out


def make_case(D, A, mb, first, seed):
    rng = np.random.default_rng(seed)
    N = first + mb + 100
    params = make_params(D, A, rng)
    teacher = make_params(D, A, rng)
    obs = f32r(np.clip(rng.standard_normal((N, D)) * rng.uniform(0.3, 2.0, D), -CLIP_OBS, CLIP_OBS))
    tmean, _, tvalue = P.policy_forward(teacher, obs)
    tmean, tvalue = f32r(tmean + 0.1 * rng.standard_normal((N, A))), f32r(tvalue)
    tlogstd = f32r(rng.uniform(-2.0, 0.5, A))
    assert np.abs(tlogstd - params["logstd"]).min() > 0
    perm = rng.permutation(N).astype(np.int64)
    return dict(D=D, A=A, mb=mb, first=first, N=N, params=params, obs=obs, tmean=tmean, tvalue=tvalue, tlogstd=tlogstd, perm=perm,
                idx=perm[first:first + mb])


_CASES, _WANT = {}, {}


def case_by_name(name):
    """cached: built once per process, shared, never changed by a test"""
    if name not in _CASES:
        _CASES[name] = make_case(*shapes()[name])
    return _CASES[name]


def reference(name, kind, vf_coef):
    """the f64 reference's (losses, gradients) of the case's minibatch at grad_scale 1 (the scale multiplies both); cached"""
    key = (name, kind, vf_coef)
    if key not in _WANT:
        c = case_by_name(name)
        i = c["idx"]
        _WANT[key] = DR.loss_and_grads(c["params"], c["obs"][i], c["tmean"][i], c["tvalue"][i], c["tlogstd"], kind, vf_coef)
    return _WANT[key]
