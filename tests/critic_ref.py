"""f64 restatement of the asymmetric actor-critic of include/trex_policy_critic.h, written from the header's definition: the policy
net reads `obs` [n, D], the value net `obs_v` [n, Dv]; everything else is oracle/ppo_oracle.py's arithmetic, whose mlp_forward /
mlp_backward are imported, not copied. A helper, not a conftest."""
import math

import numpy as np

from oracle.ppo_oracle import LOG_2PI, mlp_backward, mlp_forward

HID = 64
PARAM_NAMES = ["pi.W1", "pi.b1", "pi.W2", "pi.b2", "pi.W3", "pi.b3", "vf.W1", "vf.b1", "vf.W2", "vf.b2", "vf.W3", "vf.b3", "logstd"]


def layout_rule(D, A, Dv=None):
    """the header's layout: the 13 blocks in order, each on a multiple of 4 floats, vf.W1 of Dv rows -> (layout, count)"""
    Dv = D if Dv is None else Dv
    shapes = [(D, HID), (HID,), (HID, HID), (HID,), (HID, A), (A,), (Dv, HID), (HID,), (HID, HID), (HID,), (HID, 1), (1,), (A,)]
    lay, o = {}, 0
    for name, sh in zip(PARAM_NAMES, shapes):
        lay[name] = (o, sh)
        o = (o + math.prod(sh) + 3) & ~3
    return lay, o


def forward(params, obs, obs_v):
    """mean [n, A], logstd [A], value [n]"""
    mean, _ = mlp_forward(params, "pi", obs)
    value, _ = mlp_forward(params, "vf", obs_v)
    return mean, params["logstd"], value[:, 0]


def normalise(rows, mean, var, clip=10.0, epsilon=1e-8):
    return np.clip((rows - mean) / np.sqrt(var + epsilon), -clip, clip)


def loss_and_grads(params, obs, obs_v, act, neglogp_old, value_old, adv, ret, cliprange=0.2, ent_coef=0.0, vf_coef=0.5):
    """oracle.ppo_oracle.ppo_loss_and_grads with the value net on obs_v: the same statements in the same order, so that
    obs_v = obs gives the same bits. -> (dict of scalars and per-sample quantities, dict of gradients)"""
    n, A = act.shape
    a = (adv - adv.mean()) / (adv.std() + 1e-8)
    mean, acts_pi = mlp_forward(params, "pi", obs)
    vout, acts_vf = mlp_forward(params, "vf", obs_v)
    v = vout[:, 0]
    logstd = params["logstd"]
    std = np.exp(logstd)
    z = (act - mean) / std
    nlp = 0.5 * np.sum(z * z, -1) + 0.5 * LOG_2PI * A + np.sum(logstd)
    ratio = np.exp(neglogp_old - nlp)
    l1, l2 = -a * ratio, -a * np.clip(ratio, 1.0 - cliprange, 1.0 + cliprange)
    pg_loss = np.mean(np.maximum(l1, l2))
    vclip = value_old + np.clip(v - value_old, -cliprange, cliprange)
    e1, e2 = (v - ret) ** 2, (vclip - ret) ** 2
    vf_loss = 0.5 * np.mean(np.maximum(e1, e2))
    entropy = np.sum(logstd + 0.5 * (LOG_2PI + 1.0))
    loss = pg_loss - ent_coef * entropy + vf_coef * vf_loss
    grads = {}
    unclipped = l1 >= l2
    inside = (ratio >= 1.0 - cliprange) & (ratio <= 1.0 + cliprange)
    dratio = np.where(unclipped, -a, np.where(inside, -a, 0.0)) / n
    dnlp = -dratio * ratio
    dmean = dnlp[:, None] * (-(z / std))
    dlogstd = np.sum(dnlp[:, None] * (1.0 - z * z), 0) - ent_coef * np.ones(A)
    mlp_backward(params, "pi", acts_pi, dmean, grads)
    grads["logstd"] = dlogstd
    dv_un = 2.0 * (v - ret)
    dv_cl = 2.0 * (vclip - ret) * ((v - value_old >= -cliprange) & (v - value_old <= cliprange))
    dv = vf_coef * 0.5 * np.where(e1 >= e2, dv_un, dv_cl) / n
    mlp_backward(params, "vf", acts_vf, dv[:, None], grads)
    return dict(loss=loss, pg_loss=pg_loss, vf_loss=vf_loss, entropy=entropy, neglogp=nlp, ratio=ratio, value=v,
                adv_normalised=a), grads
