"""States with joints on their stops, made on the CPU from the model and the f64 oracle with fixed seeds: the inputs of
tests/test_gpu_joint_limits.py (and of scripts/joint_limit_stats.py, which measures the oracle's own f32 build on them).

Index convention: states, actions and observations are in observation order; the kernel's row of a joint rides on
lane = body index (1..25). lane_of_column(model)[i] is the lane of observation column i."""
import numpy as np

J = 25
PAST = 0.03          # rad beyond the stop (sections 1, 2, 4)
LOWER, UPPER = 0, 1


def limits(model):
    oo = model["obs_order"]
    return model["q_lower"][oo], model["q_upper"][oo]


def lane_of_column(model):
    """lane (= body index, 1..25) of observation column i"""
    lane = np.asarray(model["obs_order"], int)
    assert sorted(lane.tolist()) == list(range(1, J + 1))
    return lane


def column_of_lane(model):
    """observation column of lane j (entry 0 unused)"""
    col = np.full(J + 1, -1, int)
    col[lane_of_column(model)] = np.arange(J)
    return col


def put_on_stop(state, model, col, side, past=PAST):
    lo, hi = limits(model)
    state[13 + col] = lo[col] - past if side == LOWER else hi[col] + past


def one_stop_cases():
    """(lane, side, on_floor) of the 100 states of one_stop_states, in its order"""
    return [(j, side, floor) for floor in (False, True) for side in (LOWER, UPPER) for j in range(1, J + 1)]


def one_stop_states(model, orc, seed=0):
    """One joint 0.03 rad past one stop, every other joint strictly inside its range: airborne (base of the reset pose lifted
    5 m, the others at mid-range +- 0.3 range) and on the floor (the state after reset). Joint rates 0.5 N(0, 1); the action is
    the pose clipped to the limits, so the motor of the joint on the stop targets the stop."""
    rng = np.random.default_rng(seed)
    lo, hi = limits(model)
    col = column_of_lane(model)
    s = orc.new_state()
    orc.reset(s)
    base = orc.get_state(s)
    assert np.all((base[13:38] > lo) & (base[13:38] < hi))
    states = []
    for j, side, floor in one_stop_cases():
        st = base.copy()
        if not floor:
            st[2] += 5.0
            st[13:38] = 0.5 * (lo + hi) + 0.3 * (hi - lo) * rng.uniform(-1, 1, J)
        st[38:63] = 0.5 * rng.normal(size=J)
        put_on_stop(st, model, col[j], side)
        states.append(st)
    states = np.array(states, np.float32)
    return states, np.clip(states[:, 13:38], lo.astype(np.float32), hi.astype(np.float32))


def rollout_states(model, orc, seed, n_contact=8, n_air=8, min_points=4, every=3, max_steps=600):
    """States along an oracle rollout from reset under uniform random actions, one every third step: the first n_contact with
    at least min_points contact points and the first n_air without any."""
    rng = np.random.default_rng(seed)
    lo, hi = limits(model)
    s = orc.new_state()
    orc.reset(s)
    contact, air = [], []
    for t in range(max_steps):
        orc.step(s, rng.uniform(lo, hi))
        if t % every == every - 1:
            nc = len(orc.contacts(s)[0])
            if nc >= min_points and len(contact) < n_contact:
                contact.append(orc.get_state(s))
            elif nc == 0 and len(air) < n_air:
                air.append(orc.get_state(s))
        if len(contact) >= n_contact and len(air) >= n_air:
            break
    assert len(contact) >= n_contact and len(air) >= n_air, (len(contact), len(air))
    return np.array(contact + air)


def several_stop_states(model, orc, seed=5, ks=(1, 2, 4, 8), **kw):
    """On every rollout state, k in ks randomly chosen joints 0.03 rad past a randomly chosen stop, and a uniform random
    action. Returns states, actions, and the (columns, sides) put on a stop per state."""
    rng = np.random.default_rng(seed + 1000)
    lo, hi = limits(model)
    states, acts, placed = [], [], []
    for b in rollout_states(model, orc, seed, **kw):
        for k in ks:
            st = b.copy()
            cols = rng.choice(J, size=k, replace=False)
            sides = rng.integers(0, 2, size=k)
            for c, sd in zip(cols, sides):
                put_on_stop(st, model, c, sd)
            states.append(st)
            acts.append(rng.uniform(lo, hi))
            placed.append((cols, sides))
    return np.array(states, np.float32), np.array(acts, np.float32), placed


def all_stops_states(model, orc, past=0.05):
    """All 25 joints 0.05 rad past a stop, airborne at rest (the state of test_gpu_parity.py::test_joint_limit_rows with other
    sides): all upper, and two fixed random lower / upper mixes. The action pushes every joint further into its stop."""
    lo, hi = limits(model)
    rng = np.random.default_rng(9)
    states, acts = [], []
    for upper in (np.ones(J, bool), rng.integers(0, 2, J).astype(bool), rng.integers(0, 2, J).astype(bool)):
        st = np.zeros(13 + 2 * J)
        st[2], st[6] = 50.0, 1.0
        st[13:38] = np.where(upper, hi + past, lo - past)
        states.append(st)
        acts.append(np.where(upper, hi, lo))
    return np.array(states, np.float32), np.array(acts, np.float32)


def oracle_step(orc, state, action):
    """one env-step of the oracle from a float32 state and action: (obs, reward, contact points, limit rows at the end)"""
    s = orc.new_state()
    orc.set_state(s, np.asarray(state, np.float32).astype(np.float64))
    o, r, _ = orc.step(s, np.asarray(action, np.float32).astype(np.float64))
    return o, r, len(orc.contacts(s)[0]), orc.limit_rows(s)


def step_errors(g_obs, o_obs, g_rew, o_rew):
    """(|dq|, |dqd| / max(1, |qd|), |dtau| over the unsaturated joints / their largest, |dr| / max(1, |r|)) of one step"""
    ot, gt = o_obs[2 * J:], g_obs[2 * J:]
    free = np.abs(ot) < 0.999 * 3.0e5
    tau = np.abs(gt[free] - ot[free]).max() / max(1.0, np.abs(ot[free]).max()) if free.any() else 0.0
    return (np.abs(g_obs[:J] - o_obs[:J]).max(),
            np.abs(g_obs[J:2 * J] - o_obs[J:2 * J]).max() / max(1.0, np.abs(o_obs[J:2 * J]).max()),
            tau, abs(g_rew - o_rew) / max(1.0, abs(o_rew)))
