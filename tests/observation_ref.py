"""numpy f64 restatement of the observation channels (include/trex_batch.h, "observation channels"): the E extra columns of a
composed row from one env's get_state() vector and the oracle's model dict. Built on link_state_ref - the base axes are its
axes="base", URDF link 0's frame; tests/test_observation_ref.py pins it, the GPU tests compare trex_batch_compose_rows against it.

A specification here is a list of (kind, link, xyz, scale): kind a TREX_OBS_* value, link a URDF link index (EXTERNAL: the
column count)."""
import numpy as np

import link_state_ref as L

GRAVITY, BASE_LIN, BASE_ANG, BASE_HEIGHT, POINT_POS, POINT_VEL, POINT_HEIGHT, CONTACT, PREV_ACTION, EXTERNAL = range(10)
KINDS = 10
FLOOR_Z = 0.0005            # oracle.trex_model.default_params()


def width(kind, link, action_cols):
    if kind in (BASE_HEIGHT, POINT_HEIGHT, CONTACT):
        return 1
    return action_cols if kind == PREV_ACTION else int(link) if kind == EXTERNAL else 3


def extra_dim(spec, action_cols):
    return sum(width(k, l, action_cols) for k, l, _, _ in spec)


def columns(spec, action_cols):
    """[(first column, width)] of every channel, counted from column 3J"""
    out, at = [], 0
    for k, l, _, _ in spec:
        out.append((at, width(k, l, action_cols)))
        at += out[-1][1]
    return out


def channels(model, state, spec, action=None, extern=None, contact_fz=None, done=0.0, action_cols=None, floor_z=FLOOR_Z):
    """[E] f64: the channel columns of one env. state: get_state()'s [13 + 2J]; action: the env's action row or None; extern: its
    row of external columns; contact_fz: [num_bodies] the contact sensor's fz; done: the done column of the input row."""
    J = model["nb"] - 1
    A = J if action_cols is None else action_cols
    lb = np.asarray(model["link_body"], int)
    base_w = L.link_state(model, state, [0], axes="world")
    base_b = L.link_state(model, state, [0], axes="base")
    out, src = [], 0
    for kind, link, xyz, scale in spec:
        xyz = np.asarray(xyz, np.float32).astype(np.float64)      # (a TrexObsChannel holds the point as f32)
        if kind == GRAVITY:
            v = base_w["rotation"][0].T @ np.array([0.0, 0.0, -1.0])
        elif kind == BASE_LIN:
            v = base_b["linear_velocity"][0]
        elif kind == BASE_ANG:
            v = base_b["angular_velocity"][0]
        elif kind == BASE_HEIGHT:
            v = [base_w["position"][0][2] - floor_z]
        elif kind in (POINT_POS, POINT_VEL):
            r = L.link_state(model, state, [link], [xyz], axes="base")
            v = r["position"][0] if kind == POINT_POS else r["linear_velocity"][0]
        elif kind == POINT_HEIGHT:
            v = [L.link_state(model, state, [link], [xyz], axes="world")["position"][0][2] - floor_z]
        elif kind == CONTACT:
            v = [contact_fz[lb[link]]]
        elif kind == PREV_ACTION:
            v = np.zeros(A) if action is None or done != 0 else np.asarray(action, np.float64)
        elif kind == EXTERNAL:
            v = np.asarray(extern, np.float64)[src:src + link]
            src += link
        else:
            raise ValueError("unknown kind %r" % (kind,))
        out.append(np.asarray(v, np.float64) * scale)
    return np.concatenate(out)


def compose(model, state, spec, row, tail, **kw):
    """the composed row [3J + E + tail] from the input row [>= 3J + tail]"""
    nobs = 3 * (model["nb"] - 1)
    row = np.asarray(row, np.float64)
    return np.concatenate([row[:nobs], channels(model, state, spec, done=row[nobs + 1], **kw), row[nobs:nobs + tail]])


def obs_table(model, spec, action_cols):
    """What build_obs_table (csrc/host_tables.cpp) makes of the specification: dict of kind, body, col0, width [C] (integers), tf
    [C, 12], point [C, 3], scale [C] (f64, to be rounded to f32 by the comparison), col_chan [E], extern_cols, body_mask."""
    lb = np.asarray(model["link_body"], int)
    ltf = np.asarray(model["link_tf"], np.float64).reshape(-1, 12)
    C = len(spec)
    t = dict(kind=np.zeros(C, int), body=np.zeros(C, int), col0=np.zeros(C, int), width=np.zeros(C, int), tf=np.zeros((C, 12)),
             point=np.zeros((C, 3)), scale=np.zeros(C), col_chan=[], extern_cols=0, body_mask=0)
    at = 0
    for k, (kind, link, xyz, scale) in enumerate(spec):
        t["kind"][k], t["scale"][k], t["col0"][k] = kind, scale, at
        t["tf"][k] = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])
        if kind in (POINT_POS, POINT_VEL, POINT_HEIGHT, CONTACT):
            t["body"][k], t["tf"][k] = lb[link], ltf[link]
            t["point"][k] = ltf[link][:9].reshape(3, 3) @ np.asarray(xyz, np.float32).astype(np.float64) + ltf[link][9:]
            if kind != CONTACT:
                t["body_mask"] |= 1 << int(lb[link])
        if kind == EXTERNAL:
            t["body"][k] = t["extern_cols"]
            t["extern_cols"] += link
        t["width"][k] = width(kind, link, action_cols)
        t["col_chan"] += [k] * t["width"][k]
        at += t["width"][k]
    t["col_chan"] = np.array(t["col_chan"], int)
    return t
