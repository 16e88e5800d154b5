"""f64 numpy restatement of the floor-clearance query and the fall predicate (include/trex_batch.h: trex_batch_body_clearance,
trex_batch_set_termination), from the oracle's body poses and head position and the model arrays: hull_xyz / hull_radius /
hull_start (hull vertices with radius 0 - or, after use_primitive_collision, the sphere centres and capsule ends with their radii:
the same arrays), base_start_quat, and the parameter floor_z. A helper, not a conftest."""
import numpy as np

HEAD, TILT, CLEARANCE = 1, 2, 4


def quat_matrix(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def oracle_state(orc, state, mass_scale=None):
    s = orc.new_state()
    if mass_scale is not None:
        orc.set_domain(s, np.asarray(mass_scale, np.float64))
    orc.set_state(s, np.asarray(state, np.float64))
    return s


def world_points(model, pos, rot):
    """per body the world positions [n_b, 3] of its collision points and their radii [n_b]"""
    hs = np.asarray(model["hull_start"]).astype(int)
    out = []
    for b in range(model["nb"]):
        p = np.asarray(model["hull_xyz"], np.float64)[hs[b]:hs[b + 1]]
        r = np.asarray(model["hull_radius"], np.float64)[hs[b]:hs[b + 1]]
        out.append((p @ rot[b].T + pos[b], r))
    return out


def clearance(model, floor_z, pos, rot):
    """-> (clearance [nb], lowest [nb, 3]) from the bodies' world poses (pos [nb, 3], rot [nb, 3, 3] world <- body): the least
    (world z - radius) - floor_z over a body's collision points (+inf without points) and that point, the radius subtracted along
    z (NaN without points); among equal heights the first point"""
    nb = model["nb"]
    c, low = np.full(nb, np.inf), np.full((nb, 3), np.nan)
    for b, (w, r) in enumerate(world_points(model, pos, rot)):
        if len(w) == 0:
            continue
        h = w[:, 2] - r
        k = int(np.argmin(h))
        c[b] = h[k] - floor_z
        low[b] = (w[k, 0], w[k, 1], h[k])
    return c, low


def evaluate(orc, model, state, mass_scale=None):
    """everything the kernel reports for one state [13 + 2J]: dict(clearance [nb], lowest [nb, 3], head = head height above the
    floor, cos_tilt)"""
    s = oracle_state(orc, state, mass_scale)
    floor_z = float(orc.params["floor_z"])
    pos, rot = orc.body_poses(s)
    c, low = clearance(model, floor_z, pos, rot)
    head = float(orc.head_position(s)[2]) - floor_z
    up = quat_matrix(state[3:7]) @ quat_matrix(model["base_start_quat"]).T @ np.array([0.0, 0.0, 1.0])
    return dict(clearance=c, lowest=low, head=head, cos_tilt=float(up[2]), pos=pos, rot=rot)


def margin(clearance_row, clear_min):
    """values[2]: min over the watched bodies (clear_min not NaN) of clearance - clear_min; +inf when none is watched"""
    cm = np.asarray(clear_min, np.float64)
    w = ~np.isnan(cm)
    return float(np.min(clearance_row[w] - cm[w])) if w.any() else np.inf


def values(ev, clear_min=None):
    return np.array([ev["head"], ev["cos_tilt"], np.inf if clear_min is None else margin(ev["clearance"], clear_min)])


def reason(vals, head_height=None, max_tilt=None):
    """the reason bits of values [3] under the thresholds (None = off); the clearance criterion is values[2] < 0; strict <"""
    r = 0
    if head_height is not None and vals[0] < head_height:
        r |= HEAD
    if max_tilt is not None and vals[1] < np.cos(max_tilt):
        r |= TILT
    if vals[2] < 0:
        r |= CLEARANCE
    return r
