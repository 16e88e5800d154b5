"""The HIP-free part of the trainer's C-ABI, on the CPU and under the sanitizers: the check_policy_* functions of
csrc/host_tables.cpp - what include/trex_policy.h, trex_policy_critic.h and trex_policy_distill.h refuse before any HIP call - and
make_layout of csrc/policy_limits.h, built with csrc/model.cpp into tests/host/policy_harness.cpp by
g++ -fsanitize=address,undefined (the flags of tests/test_monitor_tables_host.py; no HIP, nothing loaded into Python) and run as a
child process, one run per case. Every refusal is asserted with its code and its WHOLE message - the text the C-ABI had before the
checks moved here, which the GPU tests match on - next to the accepting neighbour of the case; where a call is wrong twice, the
refusal that was reported first still is. No sanitizer report may appear."""
import os
import subprocess

import pytest

import critic_ref as CR
import trainer_cases as tc
from conftest import ROOT

CSRC = os.path.join(ROOT, "trex-gym_amd", "csrc")
INVALID, UNSUPPORTED = -1, -4          # TREX_E_INVALID, TREX_E_UNSUPPORTED
MSE, KL = 0, 1                         # TREX_DISTILL_MSE, TREX_DISTILL_KL
OK = "OK"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("policy_checks") / "policy_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "policy_harness.cpp"), os.path.join(CSRC, "host_tables.cpp"),
                           os.path.join(CSRC, "model.cpp")])
    return exe


@pytest.fixture
def ask(harness, tmp_path):
    def go(call, *words):
        path = os.path.join(str(tmp_path), "words.txt")
        with open(path, "w") as f:
            f.write(" ".join([call] + [w if isinstance(w, str) else repr(float(w)) for w in words]))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([harness, path], env=env, capture_output=True, text=True, timeout=120)
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        out = r.stdout.rstrip("\n")
        if out.startswith("REFUSED "):
            _, code, msg = out.split(" ", 2)
            return (int(code), msg)
        return out
    return go


NULL = (-1, 1, 0)      # a null policy


def test_create(ask):
    go = lambda n=33, D=9, A=3, hidden=64: ask("create", n, D, A, hidden)
    assert go() == OK
    assert go(n=0) == (INVALID, "num_envs must be positive") == go(n=-1) and go(n=1) == OK
    assert go(hidden=32) == (UNSUPPORTED, "the policy kernel is written for hidden = 64 (baselines' MlpPolicy)")
    for A in (0, 33):
        assert go(A=A) == (UNSUPPORTED, "act_dim must be in [1, 32]")
    for D in (0, 127):
        assert go(D=D) == (UNSUPPORTED, "obs_dim must be in [1, 126]")
    assert go(A=1) == go(A=32) == go(D=1) == go(D=126) == OK
    # wrong twice: envs before hidden before act_dim before obs_dim
    assert go(n=0, hidden=1)[1] == "num_envs must be positive"
    assert go(hidden=1, A=0)[1].startswith("the policy kernel is written for hidden = 64")
    assert go(A=0, D=0)[1] == "act_dim must be in [1, 32]"


def test_set_critic_and_the_calls_that_need_one(ask):
    assert ask("set_critic", *NULL, 5) == (INVALID, "trex_policy_set_critic: null policy")
    for dv in (-1, 127):
        assert ask("set_critic", 9, 3, 0, dv) == (INVALID, "trex_policy_set_critic: critic_dim must be in [0, 126] (0 clears)")
    assert ask("set_critic", 9, 3, 0, 0) == ask("set_critic", 9, 3, 5, 126) == OK
    assert ask("critic_stats", *NULL, 1) == ask("critic_stats", 9, 3, 5, 0) == (INVALID, "trex_policy_critic_get_stats: null argument")
    assert ask("critic_stats", 9, 3, 0, 1) == (INVALID, "trex_policy_critic_get_stats: no critic width is set (trex_policy_set_critic)")
    assert ask("critic_stats", 9, 3, 0, 0)[1].endswith("null argument") and ask("critic_stats", 9, 3, 5, 1) == OK


def test_observe(ask):
    null = (INVALID, "trex_policy_observe: null argument")
    assert ask("observe", *NULL, 1, 9, 0) == null == ask("observe", 9, 3, 0, 0, 9, 0)
    small = (INVALID, "trex_policy_observe: row_stride too small")
    assert ask("observe", 9, 3, 0, 1, 8, 0) == small and ask("observe", 9, 3, 0, 1, 9, 0) == OK          # without the reward: D
    assert ask("observe", 9, 3, 0, 1, 10, 1) == small and ask("observe", 9, 3, 0, 1, 11, 1) == OK        # with it: D + 2
    assert ask("observe", 9, 3, 0, 0, 1, 1) == null                                                      # null before the stride
    # the critic's block
    who = "trex_policy_critic_observe: "
    assert ask("critic_observe", *NULL, 1, 5) == ask("critic_observe", 9, 3, 5, 0, 5) == (INVALID, who + "null argument")
    assert ask("critic_observe", 9, 3, 0, 1, 5) == (INVALID, who + "no critic width is set (trex_policy_set_critic)")
    assert ask("critic_observe", 9, 3, 5, 1, 4) == (INVALID, who + "stride_v < critic_dim") and ask("critic_observe", 9, 3, 5, 1, 5) == OK


def act_call(theta=1, rows=1, rows_v=1, noise=1, actions=1, value_out=1, obs_v_out=1, row_stride=9, stride_v=5, value_only=0):
    return (theta, rows, rows_v, noise, actions, value_out, obs_v_out, row_stride, stride_v, value_only)


def test_act(ask):
    who = "trex_policy_act: "
    go = lambda policy=(9, 3, 0), **kw: ask("act", *policy, *act_call(**kw))
    assert go() == OK
    assert go(policy=NULL) == go(theta=0) == go(rows=0) == (INVALID, who + "null argument")
    assert go(policy=(9, 3, 5)) == (INVALID, who + "the policy has a critic width set (trex_policy_critic_act takes its row)")
    assert go(noise=0) == go(actions=0) == (INVALID, who + "noise / actions are null")
    assert go(noise=0, actions=0, value_only=1) == OK
    assert go(value_only=1, value_out=0) == (INVALID, who + "value_out is null") and go(value_out=0) == OK
    assert go(row_stride=8) == (INVALID, who + "row_stride < obs_dim") and go(row_stride=9) == go(row_stride=14) == OK
    assert go(policy=(9, 3, 5), rows=0) == (INVALID, who + "null argument")                # null before the critic width
    assert go(noise=0, row_stride=8) == (INVALID, who + "noise / actions are null")        # ... before the stride


def test_critic_act_and_its_value_only_combinations(ask):
    who = "trex_policy_critic_act: "
    go = lambda policy=(9, 3, 5), **kw: ask("critic_act", *policy, *act_call(**kw))
    assert go() == OK
    assert go(policy=NULL) == go(theta=0) == (INVALID, who + "null argument")
    assert go(policy=(9, 3, 0)) == (INVALID, who + "no critic width is set (trex_policy_set_critic)")
    # value_only: the critic's rows and value_out, nothing of the policy's
    needs = (INVALID, who + "value_only needs rows_v and value_out")
    assert go(value_only=1, rows_v=0) == go(value_only=1, value_out=0) == needs
    assert go(value_only=1, rows=0, noise=0, actions=0, obs_v_out=0) == OK
    # a rollout step: the policy's inputs; without rows_v nothing of the critic's
    nulls = (INVALID, who + "rows / noise / actions are null")
    assert go(rows=0) == go(noise=0) == go(actions=0) == nulls
    only = (INVALID, who + "without rows_v only the policy runs: value_out and obs_v_out must be null")
    assert go(rows_v=0) == go(rows_v=0, obs_v_out=0) == go(rows_v=0, value_out=0) == only
    assert go(rows_v=0, value_out=0, obs_v_out=0) == OK
    assert go(row_stride=8) == (INVALID, who + "row_stride < obs_dim") and go(row_stride=9) == OK
    assert go(stride_v=4) == (INVALID, who + "stride_v < critic_dim") and go(stride_v=5) == OK
    assert go(value_only=1, rows=0, row_stride=0) == OK and go(rows_v=0, value_out=0, obs_v_out=0, stride_v=0) == OK     # (an absent block's stride is not looked at)
    assert go(row_stride=8, stride_v=4)[1] == who + "row_stride < obs_dim"
    assert go(policy=(9, 3, 0), value_only=1, rows_v=0)[1] == who + "no critic width is set (trex_policy_set_critic)"


def test_gae_and_minibatch_stats(ask):
    bad = (INVALID, "trex_policy_gae: bad argument")
    assert ask("gae", *NULL, 1, 4) == ask("gae", 9, 3, 0, 0, 4) == ask("gae", 9, 3, 0, 1, 0) == ask("gae", 9, 3, 0, 1, -1) == bad
    assert ask("gae", 9, 3, 0, 1, 1) == OK
    bad = (INVALID, "trex_policy_minibatch_stats: bad argument")
    go = lambda policy=(9, 3, 0), buffers=1, nmb=2, mb=33, ns=66: ask("minibatch_stats", *policy, buffers, nmb, mb, ns)
    assert go() == go(nmb=1, mb=1, ns=1) == OK
    assert go(policy=NULL) == go(buffers=0) == bad
    for v in (0, -1):
        assert go(nmb=v) == go(mb=v) == go(ns=v) == bad


PPO_ENTRIES = ("trex_policy_minibatch_step", "trex_policy_minibatch_grad")
CRITIC_ENTRIES = ("trex_policy_critic_minibatch_step", "trex_policy_critic_minibatch_grad")
DISTILL_ENTRIES = ("trex_policy_distill_minibatch_step", "trex_policy_distill_minibatch_grad")


def minibatch(ask, who, policy=(9, 3, 0), buffers=1, mb=33, first=0, ns=33, kind=MSE, tlogstd=1, tvalue=1, vf_coef=0.5):
    return ask("minibatch", who, *policy, int(who in DISTILL_ENTRIES), int(who in CRITIC_ENTRIES), buffers, mb, first, ns, kind, tlogstd,
               tvalue, vf_coef)


@pytest.mark.parametrize("who", PPO_ENTRIES + CRITIC_ENTRIES + DISTILL_ENTRIES)
def test_what_every_minibatch_entry_point_refuses(ask, who):
    base = (9, 3, 5) if who in CRITIC_ENTRIES else (9, 3, 0)
    go = lambda **kw: minibatch(ask, who, **dict(dict(policy=base), **kw))
    assert go() == OK
    assert go(policy=NULL) == go(buffers=0) == (INVALID, who + ": null argument")
    sizes = (INVALID, who + ": bad sizes")
    for v in (0, -1):
        assert go(mb=v) == go(ns=v) == sizes
    assert go(first=-1) == sizes and go(first=0) == go(first=5) == go(mb=1, ns=1) == OK
    assert go(buffers=0, mb=0) == (INVALID, who + ": null argument")                       # null before the sizes
    # the learner's widths: 96 columns are staged, of either net
    wide = (INVALID, who + ": the learner stages 96 observation columns (obs_dim <= 96)")
    assert go(policy=(97,) + base[1:]) == wide and go(policy=(96, 32, base[2])) == OK
    assert go(policy=(97,) + base[1:], mb=0) == sizes                                      # the sizes before the widths
    # one trip of 256 x 13 float4s per net (no policy that trex_policy_create makes gets here: a check of the layout alone)
    trip = (INVALID, who + ": the learner stages one net's parameters in one trip of 256 x 13 float4s")
    assert go(policy=(96, 48, base[2])) == trip and go(policy=(96, 44, base[2])) == OK
    assert go(policy=(97, 48, base[2])) == wide


def test_a_minibatch_call_on_a_policy_of_the_other_kind(ask):
    for who in PPO_ENTRIES:
        assert minibatch(ask, who, policy=(9, 3, 5)) == (
            INVALID, who + ": the policy has a critic width set (the trex_policy_critic_minibatch calls take obs_v)")
    for who in CRITIC_ENTRIES:
        assert minibatch(ask, who, policy=(9, 3, 0)) == (INVALID, who + ": no critic width is set (trex_policy_set_critic)")
        wide = (INVALID, who + ": the learner stages 96 observation columns (critic_dim <= 96)")
        assert minibatch(ask, who, policy=(9, 3, 97)) == wide and minibatch(ask, who, policy=(9, 3, 96)) == OK
        assert minibatch(ask, who, policy=(97, 3, 97)) == wide                             # the critic's width before the policy's
    for who in DISTILL_ENTRIES:
        assert minibatch(ask, who, policy=(9, 3, 5)) == (
            INVALID, who + ": the policy has a critic width set (a student has no privileged critic)")


@pytest.mark.parametrize("who", DISTILL_ENTRIES)
def test_the_rules_of_distillation(ask, who):
    go = lambda **kw: minibatch(ask, who, **kw)
    kind = (INVALID, who + ": unknown loss kind (TREX_DISTILL_MSE, TREX_DISTILL_KL)")
    assert go(kind=2) == go(kind=-1) == kind and go(kind=MSE) == go(kind=KL) == OK
    assert go(kind=KL, tlogstd=0) == (INVALID, who + ": the KL loss needs teacher_logstd") and go(kind=MSE, tlogstd=0) == OK
    value = (INVALID, who + ": teacher_value may be null only with vf_coef == 0")
    assert go(tvalue=0, vf_coef=0.5) == go(tvalue=0, vf_coef=-1e-3) == value
    assert go(tvalue=0, vf_coef=0.0) == go(tvalue=1, vf_coef=0.0) == OK
    # wrong twice: sizes, kind, logstd, value, critic width, learner width - in this order
    assert go(kind=2, mb=0) == (INVALID, who + ": bad sizes")
    assert go(kind=2, tvalue=0) == kind and go(kind=2, policy=(9, 3, 5)) == kind
    assert go(kind=KL, tlogstd=0, tvalue=0)[1] == who + ": the KL loss needs teacher_logstd"
    assert go(tvalue=0, policy=(9, 3, 5)) == value
    assert go(policy=(97, 3, 5))[1] == who + ": the policy has a critic width set (a student has no privileged critic)"


@pytest.mark.parametrize("D,A,Dv", [(1, 1, 0), (75, 25, 0), (126, 32, 0), (75, 25, 40), (9, 3, 126)])
def test_make_layout_is_the_layout_rule(ask, D, A, Dv):
    from trex_gym import critic_capi
    words = ask("layout", D, A, Dv).split()
    assert words[0] == "layout"
    got = [int(x) for x in words[1:]]
    sym, sym_count = tc.layout_rule(D, A)
    want, count = critic_capi.layout_with_critic(sym, Dv or D)
    assert (want, count) == CR.layout_rule(D, A, Dv or None)
    if not Dv:
        assert (want, count) == (sym, sym_count)
    assert got == [want[k][0] for k in tc.PARAM_NAMES] + [count]
