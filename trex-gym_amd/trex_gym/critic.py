"""The privileged critic row of a TrexVecEnv, attached by attach(env, sources) (include/trex_policy_critic.h): what the value net of
an asymmetric actor-critic reads while the policy net keeps the sensors' row - the clean observation and whatever the simulator
knows and the robot will not. The critic exists during training alone: nothing of this reaches a deployed policy.

A specification is a list of Source(kind, arg); every constructor below returns such a list, so they add up:

    clean()              env.clean_obs - the observation before the sensor model (trex_gym.sensing) -, env.obs without one
    random(term, elements=None)   the draws of term `term` of the env's episode randomisation (trex_gym.randomize; an index into
                         env.randomization["terms"] or a kind name such as "friction"): one column per element - the one value of a
                         shared term, the masked bodies or joints, or all of them
    push_force()         the horizontal force (x, y) of every push term, as in effect at this step
    contact(links)       the floor-contact force (x, y, z, world axes) on the bodies of these links; the contact sensor must be on
    command()            env.commands (vx, vy, yaw rate)
    tensor(t, names=None)   a caller's [n, k] device tensor, read at every fill

    privileged(env)      the preset: clean(), then friction, push force, the shared mass scale, the foot contact forces

attach() gives the env `critic_rows` [n, Dv], `critic_names` and `critic_spec`; the rows are filled once per step and once per
reset behind the sensing launch, into preallocated buffers (the info() copies and one torch.cat(out=)), so that a captured rollout
replays. No training benefit is claimed anywhere here: that takes long runs nobody has made."""
import collections

import torch

from . import randomize_capi as RC
from ._capi import TrexError

Source = collections.namedtuple("Source", "kind arg")
MAX_WIDTH = 96            # what the native learner stages per sample and net (critic_capi.LEARNER_MAX_CRITIC_DIM)


def clean():
    return [Source("clean", None)]


def random(term, elements=None):
    return [Source("random", (term, None if elements is None else [int(e) for e in elements]))]


def push_force():
    return [Source("push_force", None)]


def contact(links):
    return [Source("contact", list(links))]


def command():
    return [Source("command", None)]


def tensor(t, names=None):
    return [Source("tensor", (t, None if names is None else list(names)))]


def flatten(spec):
    """a specification given as sources, lists of sources or a mix -> [Source]"""
    out = []
    for s in spec:
        if isinstance(s, Source):
            out.append(s)
        else:
            out += flatten(s)
    return out


def _term_index(env, term):
    terms = (env.randomization or {}).get("terms", [])
    if isinstance(term, str):
        hits = [i for i, t in enumerate(terms) if RC.KIND_NAMES[t[0]] == term]
        if not hits:
            raise ValueError("critic: the env's randomisation has no %r term" % term)
        return hits[0]
    if not 0 <= int(term) < len(terms):
        raise ValueError("critic: randomisation term %r outside [0, %d)" % (term, len(terms)))
    return int(term)


def _term_elements(env, t):
    """the element indices of values[:, t, :] that term t draws"""
    kind, mask, _, shared = env.randomization["terms"][t][:4]
    if shared or kind in (RC.FRICTION, RC.COMMAND):
        return [0]
    if kind == RC.PUSH:
        raise ValueError("critic: a push term has no per-episode draw; push_force() reads its force")
    if mask:
        return [i for i in range(RC.ELEMENTS) if mask >> i & 1]
    return list(range(min(RC.ELEMENTS, env.model.num_bodies if kind == RC.MASS else env.J)))


class _Filler:
    """The resolved sources of one env: `pieces()` refreshes the buffers that need a copy and returns the [n, k] blocks in order."""

    def __init__(self, env, sources):
        self.env, self.names, self.steps, self.recorded = env, [], [], []
        n, dev = env.num_envs, env.device
        self._values = self._push = self._wrench = None
        for s in sources:
            if s.kind == "clean":
                self._add(["obs%d" % k for k in range(env.obs_dim)],
                          lambda: env.clean_obs if env.clean_obs is not None else env.obs, ["clean", None])
            elif s.kind == "random":
                if env.random_api is None:
                    raise ValueError("critic: random(): the env has no episode randomisation (trex_gym.randomize.attach)")
                t = _term_index(env, s.arg[0])
                el = _term_elements(env, t) if s.arg[1] is None else s.arg[1]
                if any(not 0 <= e < RC.ELEMENTS for e in el):
                    raise ValueError("critic: random(): elements lie in [0, %d)" % RC.ELEMENTS)
                self._values = env.random_values
                kind = RC.KIND_NAMES[env.randomization["terms"][t][0]]
                idx = torch.tensor(el, device=dev)
                buf = torch.zeros(n, len(el), device=dev)
                self._add(["%s%d[%d]" % (kind, t, e) for e in el],
                          lambda t=t, idx=idx, buf=buf: torch.index_select(self._values[:, t], 1, idx, out=buf), ["random", [t, el]])
            elif s.kind == "push_force":
                P = env.random_api.num_pushes if env.random_api is not None else 0
                if not P:
                    raise ValueError("critic: push_force(): the env's randomisation has no push term")
                self._push = torch.zeros(n, P, 3, device=dev)
                buf = torch.zeros(n, P, 2, device=dev)
                self._add(["push%d.%s" % (p, a) for p in range(P) for a in "xy"],
                          lambda buf=buf: buf.copy_(self._push[:, :, :2]).view(n, -1), ["push_force", None])
            elif s.kind == "contact":
                bodies = [int(b) for b in env._link_bodies(s.arg)]
                try:
                    self._wrench = env.contact_wrench()
                except TrexError as e:
                    raise ValueError("critic: contact(): the contact sensor is off (env.enable_contact_sensor())") from e
                idx = torch.tensor(bodies, device=dev)
                buf, force = torch.zeros(n, len(bodies), 6, device=dev), torch.zeros(n, len(bodies), 3, device=dev)
                self._add(["contact%d.%s" % (b, a) for b in bodies for a in "xyz"],
                          lambda idx=idx, buf=buf, force=force: force.copy_(torch.index_select(self._wrench, 1, idx, out=buf)[:, :, :3]).view(n, -1),
                          ["contact", [int(env._links.index(l)) for l in s.arg]])
            elif s.kind == "command":
                if env.commands is None:
                    raise ValueError("critic: command(): the env has no commands (reward terms or command randomisation)")
                self._add(["command.vx", "command.vy", "command.yaw"], lambda: env.commands, ["command", None])
            elif s.kind == "tensor":
                t, names = s.arg
                if not hasattr(t, "dim") or t.dim() != 2 or t.shape[0] != n or t.device != dev:
                    raise ValueError("critic: tensor(): expected a [%d, k] tensor on %s" % (n, dev))
                names = ["tensor%d" % k for k in range(t.shape[1])] if names is None else names
                if len(names) != t.shape[1]:
                    raise ValueError("critic: tensor(): %d names for %d columns" % (len(names), t.shape[1]))
                self._add(list(names), lambda t=t: t, ["tensor", int(t.shape[1])])
            else:
                raise ValueError("critic: unknown source kind %r" % (s.kind,))

    def _add(self, names, step, recorded):
        self.names += names
        self.steps.append(step)
        self.recorded.append(recorded)

    def pieces(self):
        env = self.env
        if self._values is not None or self._push is not None:
            env.random_api.info(values=self._values, push_force=self._push)
        if self._wrench is not None:
            env.contact_wrench(self._wrench)
        return [step() for step in self.steps]


def attach(env, sources):
    """Give the env a critic row: `critic_rows` [n, Dv] f32, refilled behind every step_tensor and reset_tensor (and once here),
    `critic_names`, one per column, and `critic_spec` = dict(sources=, dim=, left_out=): plain data, what a checkpoint stores (a
    tensor() source is recorded by its width). sources None takes it all off again. ValueError: a source the env cannot supply, or
    no column at all, or more than 126 (the policy object's limit; the native learner trains 96)."""
    if sources is None:
        env.critic_rows, env.critic_names, env.critic_spec, env._critic_fill = None, [], None, None
        return env
    filler = _Filler(env, flatten(sources))
    dv = len(filler.names)
    if not 1 <= dv <= 126:
        raise ValueError("critic: %d columns; a critic row has 1 to 126" % dv)
    rows = torch.zeros(env.num_envs, dv, device=env.device)

    def fill():
        torch.cat(filler.pieces(), dim=1, out=env.critic_rows)

    env.critic_rows, env.critic_names = rows, list(filler.names)
    env.critic_spec = dict(sources=[list(r) for r in filler.recorded], dim=dv, left_out=[])
    env._critic_fill = fill
    fill()
    return env


def privileged(env, max_width=MAX_WIDTH):
    """The preset: clean() first, then friction, the push force (x, y), the shared mass scale and the foot contact forces, in that
    order - each where the env has it. A source is taken whole or not at all: those that no longer fit in max_width columns are
    left out and named in critic_spec["left_out"]. -> the env, attached."""
    from .termination import foot_links
    cand = [("clean", clean())]
    terms = (env.randomization or {}).get("terms", []) if getattr(env, "randomization", None) else []
    if any(t[0] == RC.FRICTION for t in terms):
        cand.append(("friction", random("friction")))
    if any(t[0] == RC.PUSH for t in terms):
        cand.append(("push_force", push_force()))
    shared_mass = [i for i, t in enumerate(terms) if t[0] == RC.MASS and t[3]]
    if shared_mass:
        cand.append(("mass", random(shared_mass[0])))
    try:
        env.contact_wrench()
        cand.append(("foot_contact", contact(foot_links(env))))
    except TrexError:
        pass
    taken, left, width = [], [], 0
    for name, src in cand:
        w = len(_Filler(env, src).names)
        if width + w <= max_width:
            taken += src
            width += w
        else:
            left.append(name)
    if not taken:
        raise ValueError("critic: nothing fits in %d columns" % max_width)
    attach(env, taken)
    env.critic_spec["left_out"] = left
    return env


PRESETS = {"clean": lambda env: attach(env, clean()), "privileged": privileged}
