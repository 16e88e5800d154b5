"""The sweep loops of the step kernel, one per solve shape, and the point-slot dispatch, bitwise against the general loop (run
with -m gpu on an MI355X).

The product instantiations choose a sweep loop once per substep - M (no joint on a stop, no point rows), P (no joint on a stop,
point rows), G (the general loop) - and reach the live point slots by a computed jump; the diagnostics instantiation
(trex_batch_debug_step) always runs G with the point slots walked one by one. Same rows visited in the same order with the same
instructions: every comparison here is equality of bits, observation columns and state, between the product step (pair launch at
n = 2, single-env launch at n = 3, step_many at S = 3) and the diagnostics step on the same states and actions.

States (CPU, fixed seeds; qualified below by the f64 oracle's contact points per substep and its limit rows after the step, and
on the device by the diagnostics dump of env 0: debug[128] = contact points, debug[129] = lim_mask of the last substep):
  airborne       fallen episode 3 (tests/episode_cases.py), its first case without a point in any substep              -> M
  resting        the landing of tests/state_sets.py, entry 22: on 4 points in every substep, no joint on a stop        -> P
  on_stop        tests/joint_limit_states.py several_stop_states, entry 4: ONE joint 0.03 rad past a stop, 8 points    -> G
  landing        fallen episode 3, age 241: no point in the first substep, then 1, 2, 2, 3          -> M, then P in one step
  twelve         the landing, entry 16: 12 points in every substep - the most any substep of these sets reaches (slots 1 .. 12)
  fallen_twelve  fallen episode 3, age 741: 10, 10, 12, 12, 12 points
Env 0 of a batch holds the case named, env k the k-th case after it in that list, so that a pair workgroup runs two shapes side
by side.

The warm start: trex_batch_debug_step is refused for a warm batch (the diagnostics kernel has no record, include/trex_batch.h),
so no in-tree run of loop G exists for a warm solve. What is checked on a warm batch in contact - every solve overwrites the
record, so it is non-empty from the second substep on -: the pair launch and the single-env launch agree bitwise over two
env-steps, and the warm rows are not the cold ones."""
import numpy as np
import pytest
import torch

import episode_cases as ec
import feature_cases as fc
import joint_limit_states as L
from gpu_support import DEV, make_vec, same_bits
from parity_helpers import oracle_wrench
from state_sets import landing_states

pytestmark = pytest.mark.gpu
J = 25
NAMES = ["airborne", "resting", "on_stop", "landing", "twelve", "fallen_twelve"]


@pytest.fixture(scope="module")
def cases():
    """name -> dict(state f32 [63], action f32 [25], counts = the f64 oracle's contact points per substep, nlim = its limit rows
    after the step)"""
    b = fc.trex()
    fallen = {c["origin"]: c for c in ec.episode(b, 3, False)}

    def qualified(state, action):
        s = b.o64.new_state()
        b.o64.set_state(s, np.asarray(state, np.float32).astype(np.float64))
        counts = []
        oracle_wrench(b.o64, b.om, None, np.asarray(action, np.float32), oracle_state=s, counts=counts)
        return dict(state=np.asarray(state, np.float32), action=np.asarray(action, np.float32), counts=counts,
                    nlim=b.o64.limit_rows(s))

    out = {}
    for c in fallen.values():
        q = qualified(c["state"], c["action"])
        if max(q["counts"]) == 0 and q["nlim"] == 0:
            out["airborne"] = q
            break
    ls, la = landing_states(b.o64, b.om)
    out["resting"] = qualified(ls[22], la[22])
    states, acts, placed = L.several_stop_states(b.om, b.o64, seed=5, n_contact=12, n_air=8)
    assert len(placed[4][0]) == 1
    out["on_stop"] = qualified(states[4], acts[4])
    out["landing"] = qualified(fallen["episode 3 age 241"]["state"], fallen["episode 3 age 241"]["action"])
    out["twelve"] = qualified(ls[16], la[16])
    out["fallen_twelve"] = qualified(fallen["episode 3 age 741"]["state"], fallen["episode 3 age 741"]["action"])
    out["_limits"] = L.limits(b.om)
    return out


def test_the_cases_are_what_they_claim(cases):
    c = cases
    assert max(c["airborne"]["counts"]) == 0 and c["airborne"]["nlim"] == 0
    assert c["resting"]["counts"] == [4] * 5 and c["resting"]["nlim"] == 0
    assert c["on_stop"]["nlim"] == 1 and c["on_stop"]["counts"] == [8] * 5
    assert c["landing"]["counts"] == [0, 1, 2, 2, 3] and c["landing"]["nlim"] == 0
    assert c["twelve"]["counts"] == [12] * 5 and c["twelve"]["nlim"] == 0
    assert c["fallen_twelve"]["counts"] == [10, 10, 12, 12, 12] and c["fallen_twelve"]["nlim"] == 0


def batch_of(cases, name, n):
    """(states [n, 63], actions [n, 25]): env 0 holds `name`, env k the k-th case after it"""
    k0 = NAMES.index(name)
    pick = [cases[NAMES[(k0 + k) % len(NAMES)]] for k in range(n)]
    return np.array([p["state"] for p in pick]), np.array([p["action"] for p in pick])


def loaded(states, **kw):
    v = make_vec(len(states), **kw)
    v.batch.set_wave_balance(1)
    v.reset_tensor()
    v.set_state(torch.tensor(states))
    assert v.batch.launch_info()["block"] == (128 if len(states) % 2 == 0 else 64)
    return v


def diagnostics_steps(states, action_steps):
    """the diagnostics step on a batch of its own, once per action block: (obs of every step, state after the last, dump of the last)"""
    v = loaded(states)
    n = len(states)
    obs, dbg = torch.zeros(n, 3 * J, device=DEV), torch.zeros(4096, device=DEV)
    out = []
    for a in action_steps:
        dbg.zero_()
        v.batch.debug_step(a.contiguous(), obs, dbg)
        out.append(obs.clone())
    state = v.get_state().clone()
    torch.cuda.synchronize()
    v.close()
    return out, state, dbg.cpu().numpy()


@pytest.mark.parametrize("n", [2, 3], ids=["pair", "single"])
@pytest.mark.parametrize("name", NAMES)
def test_product_step_equals_the_diagnostics_step(name, n, cases):
    states, acts = batch_of(cases, name, n)
    a = torch.tensor(acts, device=DEV)
    want_obs, want_state, dbg = diagnostics_steps(states, [a])
    # the last substep of env 0 on the device is the shape the case is there for
    nc, lim = int(dbg[128]), int(dbg[129])
    assert nc == cases[name]["counts"][-1], (name, nc, cases[name]["counts"])
    assert (lim != 0) == (name == "on_stop"), (name, lim)
    if name == "on_stop":
        assert lim & (lim - 1) == 0      # one joint
    v = loaded(states)
    obs, _, _ = v.step_tensor(a)
    state = v.get_state()
    assert torch.isfinite(obs).all() and not v.rows[:, 3 * J + 1].any()      # nothing was contained
    assert same_bits(obs, want_obs[0]), (name, n, "rows")
    assert same_bits(state, want_state), (name, n, "state")
    v.close()


def test_step_many_equals_the_diagnostics_steps(cases):
    """S = 3 env-steps in one launch, one env per case: each step's rows, and the state after the last"""
    S = 3
    states, acts = batch_of(cases, "airborne", len(NAMES))
    rng = np.random.default_rng(7)
    lo, hi = cases["_limits"]
    later = rng.uniform(lo, hi, (S - 1, len(NAMES), J)).astype(np.float32)
    a = torch.tensor(np.concatenate([acts[None], later]), device=DEV).contiguous()
    want_obs, want_state, _ = diagnostics_steps(states, list(a))
    v = loaded(states)
    rows = v.step_many_tensor(a)
    assert tuple(rows.shape[:2]) == (S, len(NAMES))
    for s in range(S):
        assert same_bits(rows[s][:, :3 * J], want_obs[s]), ("step", s)
    assert same_bits(v.get_state(), want_state)
    v.close()


def test_warm_batch_pair_and_single_agree(cases):
    """A warm batch in contact (record non-empty after its first solve): pair and single-env launch bitwise over two env-steps, and
    not the cold rows. See the module docstring for why the diagnostics step is not the reference here."""
    names = ["twelve", "landing", "resting", "on_stop", "fallen_twelve"]
    st = np.array([cases[k]["state"] for k in names])
    ac = np.array([cases[k]["action"] for k in names])
    runs = {}
    for kind, n, kw in (("pair", 6, dict(params={"warmstart": 0.85})), ("single", 7, dict(params={"warmstart": 0.85})), ("cold", 6, {})):
        idx = np.arange(n) % len(names)
        v = loaded(st[idx], **kw)
        a = torch.tensor(ac[idx], device=DEV)
        rows = []
        for _ in range(2):
            v.step_tensor(a)
            rows.append(v.rows.clone())
        runs[kind] = (rows, v.get_state().clone())
        v.close()
    for t in range(2):
        assert torch.isfinite(runs["pair"][0][t]).all()
        assert same_bits(runs["pair"][0][t], runs["single"][0][t][:6]), t
    assert same_bits(runs["pair"][1], runs["single"][1][:6])
    assert not same_bits(runs["pair"][0][0], runs["cold"][0][0])
