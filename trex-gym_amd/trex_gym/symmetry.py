"""Mirror symmetry of a TrexVecEnv's robot for the device trainer (include/trex_symmetry.h states every map; symmetry_capi binds it):
what "the mirrored state, observation row and action" are for the compiled model and the row layout in force, as tables checked
against the model and kept on the device.

    mirror = Mirror(env)                   # the model's pairing, the tables of env.rows, of the policy's input and of an action row
    mirror.rows(env.rows)                  # ONE launch: the mirrored rows
    mirror.actions(a), mirror.command(c), mirror.state(env.get_state())
    MirrorPPO(env, mirror, nsteps=32, ...) # PPO on the rollout and its mirror image (symmetry="augment")

A legged asset is never exactly symmetric: Mirror reports the model's residuals (masses, joint origins, axes, centres of mass) once
and refuses only a model that has no pairing at all. No training benefit is claimed for any of this."""
import numpy as np
import torch

from . import observations as O
from . import symmetry_capi as S
from .ppo import PPO


def quat_to_matrix(q):
    """[n, 4] xyzw -> [n, 3, 3]"""
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def matrix_to_quat(m):
    """[n, 3, 3] -> [n, 4] xyzw with w >= 0: of the four Shepperd forms the one with the largest divisor, per row"""
    m00, m11, m22 = m[..., 0, 0], m[..., 1, 1], m[..., 2, 2]
    d = torch.stack([1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22, 1 + m00 + m11 + m22], -1).clamp_min(0).sqrt() * 2
    a, b, c = m[..., 2, 1] - m[..., 1, 2], m[..., 0, 2] - m[..., 2, 0], m[..., 1, 0] - m[..., 0, 1]
    p, q, r = m[..., 0, 1] + m[..., 1, 0], m[..., 0, 2] + m[..., 2, 0], m[..., 1, 2] + m[..., 2, 1]
    forms = torch.stack([torch.stack([0.25 * d[..., 0], p / d[..., 0], q / d[..., 0], a / d[..., 0]], -1),
                         torch.stack([p / d[..., 1], 0.25 * d[..., 1], r / d[..., 1], b / d[..., 1]], -1),
                         torch.stack([q / d[..., 2], r / d[..., 2], 0.25 * d[..., 2], c / d[..., 2]], -1),
                         torch.stack([a / d[..., 3], b / d[..., 3], c / d[..., 3], 0.25 * d[..., 3]], -1)], -2)
    best = d.argmax(-1)
    out = torch.gather(forms, -2, best[..., None, None].expand(best.shape + (1, 4))).squeeze(-2)
    return torch.where(out[..., 3:4] < 0, -out, out)


class Mirror:
    """The mirror tables of `env` (a TrexVecEnv) on its device. lateral: the axis of URDF link 0's frame normal to the sagittal
    plane, None to search for it. external: (src, sign) over the EXTERNAL columns of the row, required where the env has such
    channels. Attributes: lateral, pair, sign (joints, observation order), body_pair, residual; row_table (the whole row of
    env.rows), obs_table (its first obs_dim columns: what the policy reads), act_table, command_table (host arrays)."""

    def __init__(self, env, lateral=None, tol_pos=5e-3, external=None, log=print):
        self.device = env.device
        dev = env.device.index or 0
        t = S.model_mirror_table(env.model, lateral, tol_pos)
        self.lateral, self.pair, self.sign, self.body_pair, self.residual = t["lateral"], t["pair"], t["sign"], t["body_pair"], t["residual"]
        self.J, self.A = int(env.J), int(env.A)
        chans = []
        if getattr(env, "observations", None):
            chans = O.resolve(O.from_tuples(env.observations), env._links.index, self.A)[0]
        tail = 5 if getattr(env, "_pen_in_rows", False) else 2
        es, eg = (None, None) if external is None else external
        src, sign = S.row_table(env.model, chans, self.A, tail, self.lateral, tol_pos, es, eg)
        self.width, self.obs_dim = len(src), len(src) - tail
        rows = getattr(env, "rows", None)
        if rows is not None and int(rows.shape[-1]) != self.width:     # the row in force is the batch's: the tables must fit it
            raise ValueError("Mirror: the tables describe a row of %d columns, env.rows has %d (channels or penalties set behind "
                             "the env's construction?)" % (self.width, int(rows.shape[-1])))
        self.row_table = S.MirrorTable(src, sign, dev)
        self.obs_table = S.MirrorTable(src[:self.obs_dim], sign[:self.obs_dim], dev)
        self.act_table = S.MirrorTable(*S.action_table(self.pair, self.sign, self.A == 2 * self.J), device=dev)
        self.command_table = S.command_table(self.lateral)
        self.critic_table = None             # MirrorPPO(critic=True) builds it from critic_rules
        self._link_tf = np.asarray(env.model.array("link_tf"), np.float64).reshape(-1, 12)[0]
        if log:
            log("mirror: lateral axis %d of link 0; not symmetric by  " % self.lateral + "  ".join("%s %.3g" % kv for kv in self.residual.items()))

    def critic_rules(self, env, tensor_rules=None, world_axis=0):
        """(src, sign) of the env's critic row (trex_gym.critic.attach) from its recorded sources, one rule per source kind:
          clean       the observation table
          random      MASS: a body's scale goes to the paired body's; KP, KD, MAX_FORCE: a joint's factor to the paired joint's;
                      FRICTION, a shared draw: unchanged; COMMAND: the component's sign of the command table. The partner of a
                      drawn element must be drawn too, else ValueError.
          push_force  the world force (x, y) of the push on a body goes to the push on the PAIRED body, x y as a polar vector of
                      the world reflected in `world_axis`; a body whose partner has no push term: ValueError
          contact     the world force on a body goes to the paired body's columns, polar; a partner not listed: ValueError
          command     the command table
          tensor      tensor_rules: one (src, sign) per tensor source, in order, over that tensor's columns; none: ValueError
        """
        from . import randomize_capi as RC
        spec = getattr(env, "critic_spec", None)
        if spec is None:
            raise ValueError("Mirror: the env has no critic row (trex_gym.critic.attach)")
        src, sign, rules = [], [], list(tensor_rules or [])
        polar = [-1 if k == world_axis else 1 for k in range(3)]
        body_link = lambda l: int(env._links.link_body[l])

        def block(local_src, local_sign):
            at = len(src)
            src.extend(at + int(c) for c in local_src)
            sign.extend(int(g) for g in local_sign)

        def partners(items, pair_of, what):
            out = []
            for it in items:
                p = pair_of(it)
                if p not in items:
                    raise ValueError("Mirror: critic %s: %r is drawn, its mirror partner %r is not" % (what, it, p))
                out.append(items.index(p))
            return out
        for kind, arg in spec["sources"]:
            if kind == "clean":
                block(self.obs_table.src, self.obs_table.sign)
            elif kind == "command":
                block(*self.command_table)
            elif kind == "random":
                t, el = arg
                term = env.randomization["terms"][t]
                k, index, shared = term[0], term[2], term[3]
                if k == RC.COMMAND:
                    block([0], [self.command_table[1][int(index)]])
                elif shared or k == RC.FRICTION:
                    block(range(len(el)), [1] * len(el))
                elif k == RC.MASS:
                    block(partners(list(el), lambda b: int(self.body_pair[b]), "random(mass)"), [1] * len(el))
                else:
                    block(partners(list(el), lambda j: int(self.pair[j]), "random(%s)" % RC.KIND_NAMES[k]), [1] * len(el))
            elif kind == "push_force":
                bodies = [int(t[2]) for t in env.randomization["terms"] if t[0] == RC.PUSH]
                p = partners(bodies, lambda b: int(self.body_pair[b]), "push_force")
                block([2 * q + a for q in p for a in range(2)], polar[:2] * len(p))
            elif kind == "contact":
                bodies = [body_link(l) for l in arg]
                p = partners(bodies, lambda b: int(self.body_pair[b]), "contact")
                block([3 * q + a for q in p for a in range(3)], polar * len(p))
            elif kind == "tensor":
                if not rules:
                    raise ValueError("Mirror: a tensor() source of the critic row needs a caller rule (tensor_rules)")
                r_src, r_sign = rules.pop(0)
                if sorted(int(c) for c in r_src) != list(range(int(arg))) or len(r_sign) != int(arg):
                    raise ValueError("Mirror: the rule of a tensor() source of %d columns must permute them" % int(arg))
                block(r_src, r_sign)
            else:
                raise ValueError("Mirror: no mirror rule for the critic source %r" % (kind,))
        assert len(src) == int(spec["dim"])
        return np.array(src, np.int32), np.array(sign, np.int8)

    def tables(self):
        """what a checkpoint keeps: plain lists"""
        return dict(lateral=int(self.lateral), pair=self.pair.tolist(), sign=self.sign.tolist(), row_src=self.row_table.src.tolist(),
                    row_sign=self.row_table.sign.tolist(), obs_dim=self.obs_dim, residual={k: float(v) for k, v in self.residual.items()})

    def rows(self, x, out=None, stream=None):
        """the mirror image of rows [n, obs_dim] (the policy's input) or [n, >= width] (env.rows); out None: a new tensor, out is x:
        in place"""
        table = self.obs_table if x.shape[-1] == self.obs_dim else self.row_table
        return table.rows(x, out, stream=stream)

    def actions(self, a, out=None, stream=None):
        return self.act_table.rows(a, out, stream=stream)

    def command(self, c):
        """(vx, vy, wz) in base axes -> its image (torch or numpy, any leading shape)"""
        src, sign = self.command_table
        sg = torch.as_tensor(sign, dtype=c.dtype, device=c.device) if torch.is_tensor(c) else sign.astype(np.asarray(c).dtype)
        return c[..., src.tolist()] * sg

    def symmetric_action(self, agent, rows=None, out=None):
        """(mu(s) + M_a mu(M_o s)) / 2 for the rows s (default: the env's) under the policy of `agent` (a PPO): two act calls with
        zero noise - the action is the mean - and the two row launches. Equivariant bit for bit:
        symmetric_action(M_o s) == M_a symmetric_action(s). What --play --symmetric steps the env with."""
        k, n = agent.kern, agent.env.num_envs
        rows = agent.env.rows if rows is None else rows
        zero = torch.zeros(n, k.A, device=rows.device)
        a, b = torch.empty(n, k.A, device=rows.device), torch.empty(n, k.A, device=rows.device)
        k.act(agent.policy.theta, rows, zero, a, clip_obs=agent.clip_obs)
        k.act(agent.policy.theta, self.rows(rows.contiguous()), zero, b, clip_obs=agent.clip_obs)
        out = torch.empty_like(a) if out is None else out
        torch.add(a, self.actions(b), out=out)
        return out.mul_(0.5)

    def state(self, states, world_axis=0):
        """The mirror image of states [n, 13 + 2 J] (get_state's layout) in torch, f64 inside. Defined through URDF link 0's pose:
        its position reflected in the world axis `world_axis` (S_w), its orientation S_w R S_l with S_l the reflection of link 0's
        lateral axis, linear velocity polar, angular velocity axial, q and qd through the joint table; body 0's frame sits at the
        fixed offset link_tf[0] from link 0's, and that offset is carried exactly. With lateral 0, world_axis 0 and body 0's frame
        aligned with link 0's the quaternion rule is (x, -y, -z, w)."""
        s = states.to(torch.float64)
        J, dev = self.J, s.device
        L = torch.tensor(self._link_tf[:9].reshape(3, 3), dtype=torch.float64, device=dev)
        tL = torch.tensor(self._link_tf[9:], dtype=torch.float64, device=dev)
        Sw, Sl = torch.ones(3, dtype=torch.float64, device=dev), torch.ones(3, dtype=torch.float64, device=dev)
        Sw[world_axis], Sl[self.lateral] = -1.0, -1.0
        Rb = quat_to_matrix(s[:, 3:7])
        off = Rb @ tL
        w = s[:, 10:13]
        pl, vl = s[:, 0:3] + off, s[:, 7:10] + torch.linalg.cross(w, off)
        Rl2 = Sw[None, :, None] * (Rb @ L) * Sl[None, None, :]
        Rb2 = Rl2 @ L.T
        off2, w2 = Rb2 @ tL, -(Sw * w)
        pair = torch.as_tensor(self.pair.astype(np.int64), device=dev)
        sg = torch.as_tensor(self.sign.astype(np.float64), device=dev)
        out = torch.cat([Sw * pl - off2, matrix_to_quat(Rb2), Sw * vl - torch.linalg.cross(w2, off2), w2,
                         s[:, 13:13 + J][:, pair] * sg, s[:, 13 + J:13 + 2 * J][:, pair] * sg], 1)
        return out.to(states.dtype)


def mirrored_clip(clip, mirror, world_axis=0):
    """The mirror image of a trex_gym.motion.Clip under `mirror` (a Mirror of the clip's model), built on mirror.state: every
    frame's pose and velocity mirrored. A looping clip - whose last frame is the first, moved on by the cycle's displacement - is
    also shifted by half a cycle (DeepMimic's mirror: the image of a left step starts where the clip takes its right step), the
    displacement carried over the seam; an odd cycle shifts by (F - 1) // 2 frames. A function here and no method of Clip: the
    members of Clip are recorded by an existing test."""
    from .motion import Clip
    F, J = clip.num_frames, clip.num_joints
    st = np.zeros((F, 13 + 2 * J))
    st[:, :7], st[:, 13:13 + J] = clip.frames[:, :7], clip.frames[:, 7:]
    if clip.velocities is not None:
        st[:, 7:13], st[:, 13 + J:] = clip.velocities[:, :6], clip.velocities[:, 6:]
    im = mirror.state(torch.as_tensor(st, dtype=torch.float64), world_axis).cpu().numpy()
    if clip.loop:
        P, h = F - 1, (F - 1) // 2
        disp = im[P, :3] - im[0, :3]
        idx = np.arange(F) + h
        wraps = idx // P
        im = im[idx % P].copy()
        im[:, :3] += wraps[:, None] * disp          # (positions run on over the seam)
    frames = np.concatenate([im[:, :7], im[:, 13:13 + J]], 1)
    vel = None if clip.velocities is None else np.concatenate([im[:, 7:13], im[:, 13 + J:]], 1)
    return Clip(frames, clip.frame_dt, clip.loop, vel)


def clip_with_mirror(clip, mirror, world_axis=0):
    """`clip` followed in time by its mirror image (mirrored_clip), as ONE clip of 2 F frames (a looping clip: 2 F - 1, its closing
    frame is where the image starts): what --motion CLIP --mirror_clip trains on. The image is moved horizontally so that its first
    frame's base stands where the clip's last frame stands; the joint pose jumps at the seam by whatever the clip's last frame
    and the image's first differ - nothing for a looping, symmetric gait, whose image is shifted by half a cycle."""
    from .motion import Clip
    im = mirrored_clip(clip, mirror, world_axis)
    frames = im.frames.copy()
    frames[:, :2] += clip.frames[-1, :2] - frames[0, :2]
    keep = slice(1, None) if clip.loop else slice(0, None)
    vel = None if clip.velocities is None else np.concatenate([clip.velocities, im.velocities[keep]])
    return Clip(np.concatenate([clip.frames, frames[keep]]), clip.frame_dt, clip.loop, vel)


def symmetrize_theta(policy, mirror, layout):
    """Project the flat parameter vector `policy.theta` (an MlpPolicy) in place onto mirror-equivariant parameters of this form:
    the rows of both W1 averaged with their images (row c with sign[c] x row src[c]: the hidden layers become invariant), the
    columns of pi.W3, pi.b3 and logstd averaged with their images under the action table (logstd with sign +1). Then mu(M_o s) =
    mu(s) = M_a mu(s) and V(M_o s) = V(s): the mirror loss and its gradient are zero. A small subspace - it holds only policies
    whose actions are their own mirror images -, offered for tests and as a starting point. layout: Policy.layout."""
    def block(name):
        off, shape = layout[name]
        return policy.theta.data[off:off + int(np.prod(shape))].view(*shape)
    dev = policy.theta.device
    o_src = torch.as_tensor(mirror.obs_table.src.astype(np.int64), device=dev)
    o_sg = torch.as_tensor(mirror.obs_table.sign.astype(np.float32), device=dev)
    a_src = torch.as_tensor(mirror.act_table.src.astype(np.int64), device=dev)
    a_sg = torch.as_tensor(mirror.act_table.sign.astype(np.float32), device=dev)
    with torch.no_grad():
        for name in ("pi.W1", "vf.W1"):
            w = block(name)
            w.copy_((w + o_sg[:, None] * w[o_src]) * 0.5)
        w = block("pi.W3")
        w.copy_((w + a_sg[None, :] * w[:, a_src]) * 0.5)
        b = block("pi.b3")
        b.copy_((b + a_sg * b[a_src]) * 0.5)
        ls = block("logstd")
        ls.copy_((ls + ls[a_src]) * 0.5)
    return policy


class MirrorPPO(PPO):
    """PPO(env, **ppo_kw) with the robot's mirror symmetry (include/trex_symmetry.h). In every mode trex_policy_symmetrize_stats
    runs behind every observe, so that normalising commutes with mirroring.
    symmetry="augment" (rsl_rl's augmentation): the rollout buffers hold 2 T n samples; ONE trex_mirror_augment launch behind GAE
      appends the images, which keep the originals' log-probability, value, advantage and return - the rollout policy is treated
      as if it were symmetric; an epoch keeps PPO's minibatch SIZE and runs 2 x nminibatches steps, so no limit of the learner
      kernels is touched.
    symmetry="loss" (rsl_rl's mirror loss): per rollout step the rows are mirrored, a second act call with zero noise gives
      mu_old(M_o s), and its image M_a mu_old(M_o s) is the sample's target - the ROLLOUT policy's mean, a proximal target like
      every other target of the step. Per minibatch: trex_policy_minibatch_grad, then trex_policy_distill_minibatch_grad(MSE,
      vf_coef 0, grad_scale sym_coef) - the gradient of sym_coef (1 / mb) sum_i |mu(s_i) - target_i|^2 / 2 - into a second buffer,
      their sum, trex_policy_adam.
    symmetry="both": both; the mirrored samples get their own targets, M_a mu_old(s), from a third act call.
    symmetry=None is PPO, launch for launch. mirror None: Mirror(env). use_graphs=True captures all of it. critic=True goes with
    "augment": the critic rows are augmented and their moments symmetrised through Mirror.critic_rules (critic_tensor_rules: the
    caller's rules for tensor() sources); with the mirror loss critic= is refused, as it is with distillation. Refused for a
    data-parallel env. A class of its own: PPO's signature is recorded by an existing test."""

    def __init__(self, env, mirror=None, symmetry="augment", sym_coef=1.0, critic_tensor_rules=None, **ppo_kw):
        mirror = (mirror if mirror is not None else Mirror(env)) if symmetry else None
        if symmetry and ppo_kw.get("critic"):       # (the critic rows are augmented through a table of their own)
            mirror.critic_table = S.MirrorTable(*mirror.critic_rules(env, critic_tensor_rules), device=env.device.index or 0)
        self._symmetry = (symmetry, mirror, sym_coef)
        super().__init__(env, **ppo_kw)
