"""The cases of the inverse kinematics tests (tests/test_ik_cases_host.py qualifies them on the reference alone; the GPU tests
run them): task forms - which probes, which parts of them, which joints may move - and per form seeded draws of a base pose and
targets. Everything a test hands to the GPU is rounded to f32 here, so that the reference sees the same numbers.

Reachable draws: the targets are the forward kinematics of q* = clamp(q_start + 0.5 u (q_upper - q_lower) / 2), u uniform in
[-1, 1] (the joints that may not move stay at q_start), and the solve starts at q_start. Unreachable draws: the position targets at
q_start displaced by up to 1.5 m each."""
import collections

import numpy as np

import ik_ref as IK
import link_state_ref as L

OFFSET = (0.07, -0.02, 0.03)
Form = collections.namedtuple("Form", "name links points modes joints")
Case = collections.namedtuple("Case", "state q_start q_star targets")     # targets: {"world": [K, 7], "base": [K, 7]}, f32-exact


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def pick(model):
    """dict(head, toe_a, toe_b, deepest): the head link, two toes on different legs, the deepest link"""
    names, lb = list(model["link_names"]), np.asarray(model["link_body"], int)
    depth, parent = np.asarray(model["depth"], int), np.asarray(model["parent"], int)
    head = [l for l in range(len(names)) if lb[l] == int(model["head_body"])][0]
    deepest = [l for l in range(len(names)) if lb[l] == int(np.argmax(depth))][0]

    def root_child(b):
        while parent[b] > 0:
            b = parent[b]
        return b
    toes = [l for l in range(len(names)) if "toe" in names[l] and lb[l] > 0]
    if len({root_child(lb[l]) for l in toes}) < 2:      # a generated model: the deepest links of two other branches
        order = sorted(range(1, model["nb"]), key=lambda b: -depth[b])
        toes = [[l for l in range(len(names)) if lb[l] == b][0] for b in order]
        toes = [l for l in toes if l not in (head, deepest)]
    a = toes[0]
    b = ([l for l in toes if root_child(lb[l]) != root_child(lb[a])] or [l for l in toes if lb[l] != lb[a]])[0]
    return dict(head=head, toe_a=a, toe_b=b, deepest=deepest)


def chain_joints(model, link):
    """observation indices of the joints between the base and the link's body"""
    slot = np.full(model["nb"], -1)
    slot[model["obs_order"]] = np.arange(model["nb"] - 1)
    b, out = int(model["link_body"][link]), []
    while b > 0:
        out.append(int(slot[b]))
        b = int(model["parent"][b])
    return sorted(out)


def forms(model):
    p = pick(model)
    four = [p["head"], p["toe_a"], p["toe_b"], p["deepest"]]
    zero, off = (0.0, 0.0, 0.0), OFFSET
    pts4 = [zero, off, zero, off]
    leg = chain_joints(model, p["toe_a"])
    return [
        Form("pos4", four, pts4, [1, 1, 1, 1], None),                                    # M = 12
        Form("head_ori", four, pts4, [3, 1, 1, 1], None),                                # M = 15
        Form("three_ori", four, pts4, [3, 3, 3, 1], None),                               # M = 21
        Form("k1", [p["toe_a"]], [off], [1], None),                                      # K = 1, M = 3
        Form("k8", [l for l in four for _ in range(2)], [zero, off] * 4, [1] * 8, None),  # K = 8, M = 24
        Form("same_body", [p["toe_a"]] * 2, [zero, (0.2, -0.1, 0.1)], [1, 1], None),     # two points of one body: rank-deficient
        Form("one_leg", [p["toe_a"]], [off], [1], leg),                                  # only that leg's joints may move
        Form("one_leg_ori", [p["toe_a"], p["toe_b"]], [off, zero], [2, 1], leg),         # toe_b's chain is held: its target is met
    ]


def form_of(model, name):
    return [f for f in forms(model) if f.name == name][0]


def poses(model, state, q, form):
    """the form's probes at joint angles q: {"world": [K, 7], "base": [K, 7]}, rounded to f32"""
    s = IK.with_q(model, state, q)
    return {fr: f32(L.pose_array(L.link_state(model, s, form.links, form.points, axes=fr))) for fr in ("world", "base")}


def _draw(model, form, seed, reachable):
    rng = np.random.default_rng(seed)
    J = model["nb"] - 1
    oo = model["obs_order"]
    lo, hi = IK.limits(model)
    quat = rng.normal(size=4)
    quat /= np.linalg.norm(quat)
    q0 = f32(np.clip(f32(np.asarray(model["q_start"], np.float64)[oo]), lo, hi))
    state = f32(np.concatenate([rng.uniform(-1, 1, 2), [rng.uniform(4, 6)], quat, np.zeros(6), q0, np.zeros(J)]))
    move = IK.joint_mask(model, form.joints)
    u = rng.uniform(-1, 1, J)
    q_star = np.where(move, np.clip(q0 + 0.5 * u * (hi - lo) / 2, lo, hi), q0)
    if reachable:
        t = poses(model, state, q_star, form)
    else:
        t = poses(model, state, q0, form)
        d = rng.normal(size=(len(form.links), 3))
        d *= (rng.uniform(0.5, 1.5, len(form.links)) / np.linalg.norm(d, axis=1))[:, None]
        t["world"][:, :3] = f32(t["world"][:, :3] + d)
        R0, p0 = IK.base_frame(model, state)
        t["base"][:, :3] = f32((t["world"][:, :3] - p0) @ R0)
    return Case(state, q0, q_star, t)


_CACHE = {}


def reachable(model, form, n, key="trex"):
    """n draws of the form, the same for every caller"""
    k = (key, form.name, n)
    if k not in _CACHE:
        base = 1000 * (1 + [f.name for f in forms(model)].index(form.name))
        _CACHE[k] = [_draw(model, form, base + i, True) for i in range(n)]
    return _CACHE[k]


def unreachable(model, n, key="trex"):
    """(form, n draws): the four position targets at q_start, each displaced by 0.5 .. 1.5 m"""
    form = forms(model)[0]
    k = (key, "unreachable", n)
    if k not in _CACHE:
        _CACHE[k] = [_draw(model, form, 90000 + i, False) for i in range(n)]
    return form, _CACHE[k]


_REF = {}


def reference(model, form, case, frame="world", key="trex", **kw):
    """ik_ref.solve of one case, computed once per (case, frame, parameters)"""
    k = (key, form.name, case.state.tobytes(), case.targets[frame].tobytes(), frame, tuple(sorted(kw.items())))
    if k not in _REF:
        _REF[k] = IK.solve(model, case.state, form.links, form.points, form.modes, case.targets[frame], frame, case.q_start,
                           form.joints, **kw)
    return _REF[k]
