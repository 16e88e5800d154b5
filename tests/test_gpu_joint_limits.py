"""Joint-limit rows of the step kernel on the GPU (run with -m gpu on an MI355X): each joint alone on each stop, several stops
together with contacts, all 25 on the upper / on mixed stops, and the launch forms and instantiations bitwise against each
other while limit rows are live. Every comparison is the kernel against the f64 oracle on the same float32 state and action
(assert_step_close of test_gpu_parity.py at its standing tolerances: 1e-4 rad, 3e-3 max(1, |qd|_inf), torque, reward) or
torch.equal between two launches. The states come from tests/joint_limit_states.py (CPU, fixed seeds).

Why: a limit-row visit takes column j of B out of registers through a computed jump into 25 (v_fmac, s_branch) entries; one
operand bound to the wrong register is wrong only for an env that has that joint on a stop, and uniform random actions from
reset almost never put one there (0 of 300 env-steps on the oracle), so neither the 4096-env tests nor the benchmark reach
that code. The layout of the table itself (16-byte preamble, 8-byte entries) is checked by the assembler at build time.

Measured on one MI355X (pytest -s prints every figure before it asserts; profiles/r09_joint_limits.txt), error of one
env-step against the f64 oracle as max |dq| rad, |dqd| / max(1, |qd|_inf), |dtau| / max|tau| unsaturated, |dr| / max(1, |r|):
  1. one joint on one stop, 100 states:   kernel 1.92e-6  4.97e-5  2.66e-5  6.08e-5;  the oracle's f32 build 7.34e-6  4.11e-4
     5.91e-4  3.74e-4. The kernel is below a tenth of the standing tolerance in q and qd, so this section also asserts the
     tight bound 4 x max(kernel, f32 oracle): |dq| <= 2.94e-5 rad, |dqd| <= 1.64e-3 max(1, |qd|_inf) (both set by the f32
     oracle). limit_rows == 1 at the end of the step on all 100; the kernel's lim_mask is bit j on all 100.
  2. several stops with contacts, 79 of 80 states kept (1 left out on the oracle's evidence, f32 oracle 1.02e-4 rad; the
     kernel is at 2.82e-5 rad there):     kernel 9.47e-6  1.06e-4  3.52e-4  7.33e-5;  the oracle's f32 build 3.51e-5  1.66e-4
     3.96e-4  1.68e-4.
     A contact row and a limit row live together at the end of the step on 35 of the 79 (44 %), a limit row on 57.
  3. all 25 on the upper stop / two mixes: kernel 5.70e-7  1.19e-5  1.47e-5  3.55e-6;  the oracle's f32 build 1.27e-6  8.09e-6
     2.92e-4  4.53e-5.
  4. launch forms, 5 rounds x 2 steps x 256 / 257 envs: every comparison bitwise. On the oracle a limit row is live at the
     end of 64 of the 80 first steps checked (80 %), 15 of them in contact.
Two deliberately wrong kernels, built once and not kept (operands b7 / b8 of the jump table swapped; the sign of ldir flipped
at the upper stop), fail section 1 exactly where they should: joints 7 and 8 on both stops and no other (8 cases, |dq| 0.8 ..
0.97 rad), and all 50 upper-stop cases and no lower-stop case.
"""
import numpy as np
import pytest
import torch

import joint_limit_states as L
from conftest import ASSET_URDF
from gpu_support import DEV, make_vec
from parity_helpers import assert_step_close

pytestmark = pytest.mark.gpu
NB, J = 26, 25
CASES = L.one_stop_cases()
# section 1 only: 4 x the larger of (the kernel's measured worst, the f32 oracle's worst) over the 100 states - see MEASURED
TIGHT_Q, TIGHT_QD = 4 * 7.34e-6, 4 * 4.11e-4


def gpu_step(states, acts, **kw):
    """one env-step of all states as one batch: (obs, reward, contact count) on the host"""
    n = len(states)
    v = make_vec(n, **kw)
    v.reset_tensor()
    v.set_state(torch.tensor(states))
    v.step_tensor(torch.tensor(acts, device=DEV))
    cnt = torch.zeros(n, dtype=torch.int32, device=DEV)
    v.batch.contact_stats(cnt, None)
    return v.obs.cpu().numpy(), v.rew.cpu().numpy(), cnt.cpu().numpy()


def report(name, errs, who="kernel"):
    e = np.array(errs)
    print("%s: %d states, %s vs f64 oracle max |dq| %.2e  |dqd|/scale %.2e  |dtau|/scale %.2e  |dr|/max(1,|r|) %.2e"
          % ((name, len(e), who) + tuple(e.max(0))))


# ---------------------------------------------------------------- 0. observation column <-> lane
def test_lane_of_a_column_on_a_known_case(model):
    lane, col = L.lane_of_column(model), L.column_of_lane(model)
    assert [model["joint_names"][j] for j in lane] == list(model["obs_joint_names"])
    assert model["joint_names"][1] == "joint_femur_right" and col[1] == 3 and lane[3] == 1
    assert model["obs_joint_names"][0] == "joint_atlas_axis" and lane[0] == 12
    assert all(lane[col[j]] == j for j in range(1, J + 1))
    assert CASES[6] == (7, L.LOWER, False) and CASES[75 + 7] == (8, L.UPPER, True) and len(CASES) == 100


# ---------------------------------------------------------------- 1. one joint on one stop
@pytest.fixture(scope="module")
def one_stop(model, oracle64, oracle32):
    states, acts = L.one_stop_states(model, oracle64)
    obs, rew, cnt = gpu_step(states, acts)
    want = [L.oracle_step(oracle64, s, a) for s, a in zip(states, acts)]
    f32 = [L.oracle_step(oracle32, s, a) for s, a in zip(states, acts)]
    errs = [L.step_errors(obs[e], want[e][0], rew[e], want[e][1]) for e in range(len(states))]
    report("one joint on one stop", errs)
    report("one joint on one stop", [L.step_errors(f32[e][0], want[e][0], f32[e][1], want[e][1]) for e in range(len(states))],
           who="the oracle's f32 build")
    return states, acts, obs, rew, cnt, want, f32, np.array(errs)


@pytest.mark.parametrize("e", range(len(CASES)), ids=["j%02d-%s-%s" % (j, "upper" if s else "lower", "floor" if f else "air")
                                                      for j, s, f in CASES])
def test_one_joint_on_one_stop(e, one_stop, model):
    """Joint j (lane j) 0.03 rad past one stop, alone: all 75 observation columns and the reward of one env-step. A wrong
    column of B for that joint is a gross error here, so the section also holds the tight bound TIGHT_Q / TIGHT_QD."""
    states, acts, obs, rew, cnt, want, f32, errs = one_stop
    j, side, floor = CASES[e]
    c = L.column_of_lane(model)[j]
    lo, hi = L.limits(model)
    assert states[e, 13 + c] < lo[c] if side == L.LOWER else states[e, 13 + c] > hi[c]
    others = np.delete(np.arange(J), c)
    assert np.all((states[e, 13 + others] > lo[others]) & (states[e, 13 + others] < hi[others]))
    assert acts[e, c] == np.float32(lo[c] if side == L.LOWER else hi[c])       # the motor targets the stop
    o, r, nco, nlim = want[e]
    assert nlim == 1                                                           # the row is there at the end of the step
    what = "joint %d (%s) %s %s" % (j, model["joint_names"][j], "upper" if side else "lower", "floor" if floor else "air")
    assert_step_close(obs[e], o, rew[e], r, what)
    assert cnt[e] == nco, what
    # the reference alone passes with room (half the standing tolerance)
    fq, fqd, _, _ = L.step_errors(f32[e][0], o, f32[e][1], r)
    assert fq <= 0.5e-4 and fqd <= 1.5e-3, what
    assert errs[e, 0] <= TIGHT_Q and errs[e, 1] <= TIGHT_QD, (what, errs[e])


def test_limit_mask_has_the_bit_of_the_joints_lane(one_stop, model):
    """Every state alone in a one-env batch through the diagnostics step: the last substep's lim_mask (debug[129]) is
    exactly bit j."""
    from trex_gym import _capi
    states, acts = one_stop[0], one_stop[1]
    b = _capi.Batch(_capi.Model(ASSET_URDF), 1, 0)
    b.reset()
    obs, dbg = torch.zeros(1, 3 * J, device=DEV), torch.zeros(4096, device=DEV)
    for e, (j, side, floor) in enumerate(CASES):
        b.set_state(torch.tensor(states[e:e + 1], device=DEV))
        b.set_motors_enabled(True)
        dbg.zero_()
        b.debug_step(torch.tensor(acts[e:e + 1], device=DEV), obs, dbg)
        torch.cuda.synchronize()
        assert int(dbg[129].item()) == 1 << j, (j, side, floor, int(dbg[129].item()))
        assert_step_close(obs[0].cpu().numpy(), one_stop[5][e][0], what="diagnostics step, case %d" % e)
    b.close()


# ---------------------------------------------------------------- 2. several stops, mixed sides, with contacts
def test_several_stops_with_contacts(model, oracle64, oracle32):
    """20 rollout states (12 with >= 4 contact points, 8 airborne) x k = 1, 2, 4, 8 joints past a random stop, a uniform
    random action. A state is left out only on the ORACLE's evidence - its own f32 build is more than half the standing
    tolerance from its f64 build there (1 of the 80: state 75, k = 8 airborne, 1.02e-4 rad) - and at least 90 % are kept."""
    states, acts, placed = L.several_stop_states(model, oracle64, seed=5, n_contact=12, n_air=8)
    assert len(states) == 80
    obs, rew, cnt = gpu_step(states, acts)
    want, keep, errs, errs32 = [], [], [], []
    for e in range(len(states)):
        want.append(L.oracle_step(oracle64, states[e], acts[e]))
        o32, r32, _, _ = L.oracle_step(oracle32, states[e], acts[e])
        errs32.append(L.step_errors(o32, want[e][0], r32, want[e][1]))
        fq, fqd = errs32[e][:2]
        errs.append(L.step_errors(obs[e], want[e][0], rew[e], want[e][1]))
        if fq <= 0.5e-4 and fqd <= 1.5e-3:
            keep.append(e)
        else:
            print("   left out on the oracle's evidence: state %d, f32 oracle |dq| %.2e |dqd|/scale %.2e; kernel %.2e %.2e"
                  % (e, fq, fqd, errs[e][0], errs[e][1]))
    both = sum(want[e][2] > 0 and want[e][3] > 0 for e in keep)
    report("several stops with contacts", [errs[e] for e in keep])
    report("several stops with contacts", [errs32[e] for e in keep], who="the oracle's f32 build")
    print("   kept %d of %d; contact and limit row together at the end of the step: %d; a limit row: %d"
          % (len(keep), len(states), both, sum(want[e][3] > 0 for e in keep)))
    assert 10 * len(keep) >= 9 * len(states)
    for e in keep:
        o, r, nco, nlim = want[e]
        assert_step_close(obs[e], o, rew[e], r, "state %d, joints %s sides %s" % (e, placed[e][0], placed[e][1]))
        assert cnt[e] == nco, e
    assert 4 * both >= len(keep)


# ---------------------------------------------------------------- 3. all 25 on a stop: upper and mixed
def test_all_joints_on_upper_and_mixed_stops(model, oracle64, oracle32):
    """All 25 joints 0.05 rad past the upper stop, and two lower / upper mixes, airborne, motors pushing further in. Unlike
    the all-lower state of test_gpu_parity.py::test_joint_limit_rows these are well conditioned (the oracle's f32 build is
    within 1e-5 of the velocity scale): the standing tolerances hold."""
    states, acts = L.all_stops_states(model, oracle64)
    assert np.all(states[0, 13:38] > L.limits(model)[1]) and len(states) == 3
    for st in states[1:]:
        n_up = int((st[13:38] > L.limits(model)[1]).sum())
        assert 5 <= n_up <= 20 and n_up + int((st[13:38] < L.limits(model)[0]).sum()) == J
    obs, rew, cnt = gpu_step(np.repeat(states, 2, axis=0)[:5], np.repeat(acts, 2, axis=0)[:5])   # (odd: the single-env launch)
    obs2, rew2, _ = gpu_step(np.repeat(states, 2, axis=0), np.repeat(acts, 2, axis=0))          # (even: the pair launch)
    assert np.array_equal(obs2[:5], obs) and np.array_equal(rew2[:5], rew)
    errs, errs32 = [], []
    for k in range(3):
        o, r, nco, nlim = L.oracle_step(oracle64, states[k], acts[k])
        assert nlim >= 20 and nco == 0
        errs.append(L.step_errors(obs[2 * k], o, rew[2 * k], r))
        o32, r32, _, _ = L.oracle_step(oracle32, states[k], acts[k])
        errs32.append(L.step_errors(o32, o, r32, r))
    report("all 25 on a stop (upper, mix, mix)", errs)
    report("all 25 on a stop (upper, mix, mix)", errs32, who="the oracle's f32 build")
    for k in range(3):
        o, r, _, _ = L.oracle_step(oracle64, states[k], acts[k])
        assert_step_close(obs[2 * k], o, rew[2 * k], r, "all-stops state %d" % k)


# ---------------------------------------------------------------- 4. launch forms and instantiations, bitwise
N_FORM, ROUNDS = 256, 5


def round_states(model, oracle64, rnd):
    """the recipes of sections 1 and 2 with the seeds of round rnd, tiled to N_FORM + 1 envs; actions of 2 steps"""
    s1, a1 = L.one_stop_states(model, oracle64, seed=100 + rnd)
    s2, a2, _ = L.several_stop_states(model, oracle64, seed=200 + rnd, n_contact=12, n_air=8)
    states, first = np.concatenate([s1, s2]), np.concatenate([a1, a2])
    idx = np.arange(N_FORM + 1) % len(states)
    lo, hi = L.limits(model)
    second = np.random.default_rng(300 + rnd).uniform(lo, hi, (N_FORM + 1, J)).astype(np.float32)
    return len(s1), states[idx], np.stack([first[idx], second])


FORMS = {
    "plain": dict(),
    "warmstart": dict(params={"warmstart": 0.85}),
    "sensor": dict(),
    "wrench": dict(),
}


@pytest.fixture(scope="module")
def form_runs(model, oracle64):
    """Every form in the pair launch (N_FORM envs) and the single-env launch (N_FORM + 1), ROUNDS rounds of set_state + 2
    steps: rows of every step, state after every round, the sensor's output; step_many of each round in both launches."""
    gen = torch.Generator().manual_seed(44)
    w = torch.zeros(N_FORM + 1, NB, 6)
    w[:, 0, :3] = 3e3 * torch.randn(N_FORM + 1, 3, generator=gen)
    w[:, 0, 3:] = 5e2 * torch.randn(N_FORM + 1, 3, generator=gen)
    vecs = {}
    for name, kw in FORMS.items():
        for n in (N_FORM, N_FORM + 1):
            v = make_vec(n, **kw)
            v.batch.set_wave_balance(1)
            if name == "sensor":
                v.enable_contact_sensor()
            v.reset_tensor()
            if name == "wrench":
                v.set_external_wrench(w[:n])
            assert v.batch.launch_info()["block"] == (128 if n % 2 == 0 else 64)
            vecs[name, n] = v
    for n in (N_FORM, N_FORM + 1):
        v = make_vec(n)
        v.batch.set_wave_balance(1)
        v.reset_tensor()
        vecs["many", n] = v
    out = {k: dict(rows=[], state=[], sensed=[]) for k in vecs}
    inputs = []
    for rnd in range(ROUNDS):
        n1, states, acts = round_states(model, oracle64, rnd)
        inputs.append((n1, states, acts))
        for (name, n), v in vecs.items():
            v.set_state(torch.tensor(states[:n]))
            a = torch.tensor(acts[:, :n], device=DEV).contiguous()
            if name == "many":
                out[name, n]["rows"].extend(v.step_many_tensor(a).clone())
            else:
                for t in range(2):
                    v.step_tensor(a[t])
                    out[name, n]["rows"].append(v.rows.clone())
                    if name == "sensor":
                        out[name, n]["sensed"].append(v.contact_wrench().clone())
            out[name, n]["state"].append(v.get_state().clone())
    return inputs, out


@pytest.mark.parametrize("name", ["plain", "warmstart", "sensor", "wrench", "many"])
def test_pair_and_single_launch_agree_bitwise_on_limit_states(name, form_runs):
    _, out = form_runs
    pair, single = out[name, N_FORM], out[name, N_FORM + 1]
    assert len(pair["rows"]) == 2 * ROUNDS and len(pair["state"]) == ROUNDS
    for t in range(2 * ROUNDS):
        assert torch.equal(single["rows"][t][:N_FORM], pair["rows"][t]), (name, "step", t)
        assert torch.isfinite(pair["rows"][t]).all() and not pair["rows"][t][:, 3 * J + 1].any()      # nothing was contained
    for r in range(ROUNDS):
        assert torch.equal(single["state"][r][:N_FORM], pair["state"][r]), (name, "round", r)
    for t in range(len(pair["sensed"])):
        assert torch.equal(single["sensed"][t][:N_FORM], pair["sensed"][t]), (name, "sensor, step", t)


@pytest.mark.parametrize("n", [N_FORM, N_FORM + 1])
def test_instantiations_agree_on_limit_states(n, form_runs):
    """Sensor on = sensor off and step_many = the steps one by one, bitwise; the warm start and the wrench really change
    the step (they are other solves, not the plain one under another name)."""
    _, out = form_runs
    plain = out["plain", n]
    for other in ("sensor", "many"):
        for t in range(2 * ROUNDS):
            assert torch.equal(out[other, n]["rows"][t], plain["rows"][t]), (other, "step", t)
        for r in range(ROUNDS):
            assert torch.equal(out[other, n]["state"][r], plain["state"][r]), (other, "round", r)
    assert (torch.stack(out["sensor", n]["sensed"])[..., 2] > 0).any()
    for other in ("warmstart", "wrench"):
        assert any(not torch.equal(out[other, n]["rows"][t], plain["rows"][t]) for t in range(2 * ROUNDS)), other


def test_form_states_hold_limit_rows(form_runs, oracle64):
    """The oracle on the first step of every round for 16 envs (8 of the one-stop states, 8 of the several-stop states): a
    limit row is live at the end of at least half of these steps, so the equalities above are about limit rows."""
    inputs, _ = form_runs
    live, total, with_contact = 0, 0, 0
    for n1, states, acts in inputs:
        for e in list(range(3, n1, 13)) + list(range(n1 + 2, n1 + 80, 10)):
            _, _, nco, nlim = L.oracle_step(oracle64, states[e], acts[0, e])
            live += nlim > 0
            with_contact += nco > 0
            total += 1
    print("launch forms: a limit row live at the end of %d of %d first steps checked on the oracle (%d of them in contact)"
          % (live, total, with_contact))
    assert total >= 16 * ROUNDS and 2 * live >= total
