"""numpy restatement of the mirror maps (include/trex_symmetry.h), written from the header's definition and not from the C++ or the
kernels: the model table, the row, action and command tables, the three maps (rows, augment, moments) and the mirrored state. f64
throughout; the maps on rows move 32-bit words and are exact for any input. The one reference of tests/test_symmetry_*.py and
tests/test_gpu_symmetry.py. A helper, not a conftest.

`model` is the dict of oracle/trex_model.py. PLANTED mistakes - keyword flags of the builders, all off by default - exist so that
tests/test_symmetry_ref.py can show that its checks see each of them:
    wrong_sign=k      the sign of joint k (observation order) is flipped
    swapped_pair=k    joint k and its partner map to themselves instead of to each other
    unmirrored_probe  a point channel keeps its own columns instead of taking its partner's (the probe offset is not mirrored)
    axial_as_polar    BASE_ANGULAR_VELOCITY gets the polar rule
"""
import numpy as np

MAXWIDTH = 517
(PROJECTED_GRAVITY, BASE_LINEAR_VELOCITY, BASE_ANGULAR_VELOCITY, BASE_HEIGHT, POINT_POSITION, POINT_VELOCITY, POINT_HEIGHT,
 CONTACT_FORCE, PREV_ACTION, EXTERNAL) = range(10)
RESIDUALS = ("mass_rel", "origin_m", "axis_rad", "com_m", "root_com_off_plane_m")


class Refused(ValueError):
    """what the C-ABI answers with TREX_E_INVALID"""


# ---------------------------------------------------------------- the model table
def body_frames(model):
    """(R [B, 3, 3], t [B, 3]): every body's frame at q = 0 in URDF link 0's frame"""
    nb = model["nb"]
    R0, t0 = model["link_tf"][0][:9].reshape(3, 3), model["link_tf"][0][9:]
    R, t = np.zeros((nb, 3, 3)), np.zeros((nb, 3))
    R[0], t[0] = R0.T, -R0.T @ t0
    for i in range(1, nb):
        p = model["parent"][i]
        R[i] = R[p] @ model["joint_rot"][i].reshape(3, 3)
        t[i] = R[p] @ model["joint_pos"][i] + t[p]
    return R, t


def _mirror_about(model, lat, tol):
    nb, nj = model["nb"], model["nb"] - 1
    R, t = body_frames(model)
    o = t.copy()
    o[0] = 0.0
    a = np.einsum("bij,bj->bi", R, model["joint_axis"])
    c = np.einsum("bij,bj->bi", R, model["com"]) + t
    S = np.ones(3)
    S[lat] = -1.0
    body_pair = np.full(nb, -1)
    for i in range(nb):
        want = S * o[i]
        if np.linalg.norm(want - o[i]) <= tol:
            body_pair[i] = i
            continue
        d = np.linalg.norm(o - want, axis=1)
        d[i] = np.inf
        j = int(np.argmin(d))          # (the lowest index among equals)
        if d[j] > tol:
            raise Refused("body %d (%s) has no partner within tol_pos" % (i, model["body_names"][i]))
        body_pair[i] = j
    for i in range(nb):
        j = body_pair[i]
        if body_pair[j] != i:
            raise Refused("the pairing of body %d is not an involution" % i)
        if i > 0 and body_pair[model["parent"][i]] != model["parent"][j]:
            raise Refused("the parents of body %d and of its partner are not paired" % i)
    slot = np.full(nb, -1)
    slot[model["obs_order"]] = np.arange(nj)
    pair, sign, res = np.zeros(nj, np.int32), np.ones(nj, np.int8), np.zeros(5)
    for i in range(nb):
        j = body_pair[i]
        mi, mj = model["mass"][i], model["mass"][j]
        res[0] = max(res[0], abs(mi - mj) / max(mi, mj))
        res[1] = max(res[1], np.linalg.norm(o[i] - S * o[j]))
        res[3] = max(res[3], np.linalg.norm(c[i] - S * c[j]))
        if i == 0:
            continue
        aj = -(S * a[j])               # an axis reflects as an axial vector
        d = float(a[i] @ aj)
        s = -1 if d < 0.0 else 1
        res[2] = max(res[2], np.arctan2(np.linalg.norm(np.cross(a[i], aj)), abs(d)))
        lo, hi = (model["q_lower"][j], model["q_upper"][j]) if s > 0 else (-model["q_upper"][j], -model["q_lower"][j])
        if abs(model["q_lower"][i] - lo) > tol or abs(model["q_upper"][i] - hi) > tol:
            raise Refused("the limits of joint %s and of its partner's image differ by more than tol_pos" % model["joint_names"][i])
        pair[slot[i]], sign[slot[i]] = slot[j], s
    res[4] = abs(c[0][lat])
    return dict(lateral=lat, pair=pair, sign=sign, body_pair=body_pair.astype(np.int32), residual=dict(zip(RESIDUALS, res)))


def model_table(model, lateral=None, tol_pos=5e-3, wrong_sign=None, swapped_pair=None):
    """dict(lateral, pair [J], sign [J], body_pair [B], residual); lateral None searches as the header says"""
    if lateral is not None:
        out = _mirror_about(model, int(lateral), tol_pos)
    else:
        out, first, why = None, None, None
        for lat in range(3):
            try:
                m = _mirror_about(model, lat, tol_pos)
            except Refused as e:
                why = why or e
                continue
            if (m["body_pair"] != np.arange(model["nb"])).any():
                out = m
                break
            first = first or m
        out = out or first
        if out is None:
            raise Refused("no axis of link 0 is normal to a mirror plane of the model (%s)" % why)
    if wrong_sign is not None:
        out["sign"][wrong_sign] = -out["sign"][wrong_sign]
    if swapped_pair is not None:
        k, p = swapped_pair, out["pair"][swapped_pair]
        out["pair"][k], out["pair"][p] = k, p
    return out


def action_table(pair, sign, stiffness=False):
    J = len(pair)
    if not stiffness:
        return np.array(pair, np.int32), np.array(sign, np.int8)
    return np.concatenate([pair, J + np.asarray(pair)]).astype(np.int32), np.concatenate([sign, np.ones(J)]).astype(np.int8)


def command_table(lateral):
    return np.arange(3, dtype=np.int32), np.array([-1 if lateral == 0 else 1, -1 if lateral == 1 else 1, 1 if lateral == 2 else -1], np.int8)


# ---------------------------------------------------------------- the row table
def channel_width(kind, link, action_cols):
    return action_cols if kind == PREV_ACTION else link if kind == EXTERNAL else 1 if kind in (BASE_HEIGHT, POINT_HEIGHT, CONTACT_FORCE) else 3


def row_table(model, mm, channels, action_cols, tail=2, tol_pos=5e-3, extern_src=None, extern_sign=None, unmirrored_probe=False,
              axial_as_polar=False):
    """(src [W], sign [W]) of the row [q | qd | torque | channel columns | tail]; channels: (kind, link, local_xyz, scale) each"""
    nj, lat = model["nb"] - 1, mm["lateral"]
    R, t = body_frames(model)
    col0, width, ext0, ext_col, col = [], [], [], [], 3 * nj
    for k, (kind, link, xyz, scale) in enumerate(channels):
        w = channel_width(kind, link, action_cols)
        col0.append(col)
        width.append(w)
        ext0.append(len(ext_col))
        if kind == EXTERNAL:
            if extern_src is None or extern_sign is None:
                raise Refused("channel %d: an EXTERNAL channel needs extern_src and extern_sign" % k)
            ext_col += list(range(col, col + w))
        col += w
    W = col + tail
    if W > MAXWIDTH:
        raise Refused("the row is wider than %d columns" % MAXWIDTH)
    if ext_col and sorted(extern_src) != list(range(len(ext_col))):
        raise Refused("extern_src is no permutation of the EXTERNAL columns")

    def point_of(link, xyz):
        b = model["link_body"][link]
        lR, lt = model["link_tf"][link][:9].reshape(3, 3), model["link_tf"][link][9:]
        return R[b] @ (lR @ np.asarray(xyz, float) + lt) + t[b]

    def partner(k):
        kind, link, xyz, scale = channels[k]
        if kind <= BASE_HEIGHT or kind >= PREV_ACTION:
            return k
        if kind != CONTACT_FORCE and unmirrored_probe:
            return k
        x = None if kind == CONTACT_FORCE else point_of(link, xyz)
        if x is not None:
            x[lat] = -x[lat]
        for j, (kj, lj, xj, sj) in enumerate(channels):
            if kj != kind or np.float32(sj) != np.float32(scale) or mm["body_pair"][model["link_body"][link]] != model["link_body"][lj]:
                continue
            if kind == CONTACT_FORCE or np.linalg.norm(x - point_of(lj, xj)) <= tol_pos:
                return j
        raise Refused("channel %d has no mirrored channel in the specification" % k)

    src, sign = np.arange(W, dtype=np.int32), np.ones(W, np.int8)
    for b in range(3):
        src[b * nj:(b + 1) * nj] = b * nj + mm["pair"]
        sign[b * nj:(b + 1) * nj] = mm["sign"]
    a_src, a_sign = action_table(mm["pair"], mm["sign"], action_cols == 2 * nj)
    for k, (kind, link, xyz, scale) in enumerate(channels):
        p = partner(k)
        for i in range(width[k]):
            at = col0[k] + i
            src[at] = col0[p] + i
            if kind in (PROJECTED_GRAVITY, BASE_LINEAR_VELOCITY, POINT_POSITION, POINT_VELOCITY) or (kind == BASE_ANGULAR_VELOCITY and axial_as_polar):
                sign[at] = -1 if i == lat else 1
            elif kind == BASE_ANGULAR_VELOCITY:
                sign[at] = 1 if i == lat else -1
            elif kind == PREV_ACTION:
                src[at], sign[at] = col0[k] + a_src[i], a_sign[i]
            elif kind == EXTERNAL:
                src[at], sign[at] = ext_col[extern_src[ext0[k] + i]], extern_sign[ext0[k] + i]
    return src, sign


# ---------------------------------------------------------------- the three maps
def check_table(src, sign, width=None):
    """the refusals of trex_mirror_table_create; -> whether the table is an involution"""
    src, sign = np.asarray(src), np.asarray(sign)
    W = len(src) if width is None else width
    if not 1 <= W <= MAXWIDTH:
        raise Refused("width %d outside [1, %d]" % (W, MAXWIDTH))
    if sorted(src.tolist()) != list(range(W)):
        raise Refused("src is no permutation")
    if not np.isin(sign, (-1, 1)).all():
        raise Refused("a sign is neither +1 nor -1")
    return bool((src[src] == np.arange(W)).all() and (sign[src] == sign).all())


def mirror_rows(src, sign, x):
    """x [n, >= W] f32 -> [n, W] f32: word c of a row is word src[c] with its sign bit flipped where sign[c] < 0. Exact for NaN
    payloads, signed zeros and infinities: no float operation touches a value."""
    src, sign = np.asarray(src), np.asarray(sign)
    words = np.ascontiguousarray(x, np.float32).view(np.uint32)[..., src]
    return (words ^ np.where(sign < 0, np.uint32(0x80000000), np.uint32(0))).view(np.float32)


def mirror_rows_f64(src, sign, x):
    """the same map on f64 values (for the reference's own qualification)"""
    return np.asarray(x, float)[..., np.asarray(src)] * np.asarray(sign, float)


def augment(obs_t, act_t, obs, act, logp, val, adv, ret, n, critic_t=None, obs_v=None):
    """the buffers [2 n, ..] with their second halves filled; the inputs are not modified"""
    out = [np.array(b, np.float32) for b in (obs, act, logp, val, adv, ret)]
    out[0][n:2 * n] = mirror_rows(*obs_t, out[0][:n])
    out[1][n:2 * n] = mirror_rows(*act_t, out[1][:n])
    for b in out[2:]:
        b[n:2 * n] = b[:n]
    if critic_t is not None:
        v = np.array(obs_v, np.float32)
        v[n:2 * n] = mirror_rows(*critic_t, v[:n])
        out.append(v)
    return out


def symmetrize_stats(src, sign, mean, var):
    """(mean, var) in f64, every operation in the header's order; numpy rounds each to f64 and fuses nothing"""
    src = np.asarray(src)
    mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    a = np.where(np.asarray(sign) < 0, -mean[src], mean[src])
    h = (mean - a) / 2.0
    hh = h * h
    half = (var + var[src]) / 2.0
    return (mean + a) / 2.0, half + hh


# ---------------------------------------------------------------- the mirrored state
def quat_to_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def matrix_to_quat(m):
    """xyzw, w >= 0 (Shepperd's branches)"""
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        q = [(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, 0.25 * s]
    elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = np.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2]) * 2
        q = [0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s, (m[2, 1] - m[1, 2]) / s]
    elif m[1, 1] > m[2, 2]:
        s = np.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2]) * 2
        q = [(m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s, (m[0, 2] - m[2, 0]) / s]
    else:
        s = np.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1]) * 2
        q = [(m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s, (m[1, 0] - m[0, 1]) / s]
    q = np.array(q)
    return -q if q[3] < 0 else q


def mirror_state(model, mm, state, world_axis=0):
    """The mirror image of a state [pos 3 | quat xyzw 4 | v 3 | w 3 | q J | qd J] (body 0's frame: position of its origin, which is
    the base's centre of mass, world velocities). Defined through URDF link 0's pose: its position is reflected in the world axis
    `world_axis` (S_w), its orientation becomes S_w R S_l with S_l the reflection of link 0's `lateral` axis, linear velocities are
    polar, angular velocities axial, q and qd go through the joint table. body 0's frame sits at the fixed offset link_tf[0] from
    link 0's: R_b = R_l L^T, p_b = p_l - R_b t_L with (L, t_L) = link_tf[0] (body <- link)."""
    nj = model["nb"] - 1
    s = np.asarray(state, float)
    L, tL = model["link_tf"][0][:9].reshape(3, 3), model["link_tf"][0][9:]
    Sw, Sl = np.ones(3), np.ones(3)
    Sw[world_axis] = -1.0
    Sl[mm["lateral"]] = -1.0
    Rb = quat_to_matrix(s[3:7])
    Rl = Rb @ L                                   # world <- link 0
    pl = s[0:3] + Rb @ tL
    wv = s[10:13]
    vl = s[7:10] + np.cross(wv, Rb @ tL)          # velocity of link 0's origin
    Rl2 = (Sw[:, None] * Rl) * Sl[None, :]
    pl2, vl2, w2 = Sw * pl, Sw * vl, -(Sw * wv)
    Rb2 = Rl2 @ L.T
    out = s.copy()
    out[0:3] = pl2 - Rb2 @ tL
    out[3:7] = matrix_to_quat(Rb2)
    out[7:10] = vl2 - np.cross(w2, Rb2 @ tL)
    out[10:13] = w2
    out[13:13 + nj] = mirror_rows_f64(mm["pair"], mm["sign"], s[13:13 + nj])
    out[13 + nj:13 + 2 * nj] = mirror_rows_f64(mm["pair"], mm["sign"], s[13 + nj:13 + 2 * nj])
    return out
