"""Training entry point with the reference's flags (trex_train.py:24-29,113-136), driving the GPU
vec env with the on-device PPO of trex_gym.ppo instead of baselines.ppo2 + TF1.

    python -m trex_gym.trex_train --num_timesteps 5000000 --num_envs 4096

Reward weights are the training ones of the reference (distance 2e2, energy 1e-6, drift 1.0,
trex_train.py:66). --play runs the trained policy and records what a renderer needs per frame (the world poses of the 252
visual meshes); --frames DIR also writes one PNG per step, ray-cast from the collision hulls (trex_batch_render). Turning
them into a movie (the reference's ffmpeg call) stays the user's.
"""
import argparse
import math
import os
import sys

import torch

from . import actuators
from .perturb import RandomGains, RandomPushes
from .ppo import PPO
from .vec_env import TrexVecEnv

_URDF_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "assets", "trex_collide.urdf")


def build_environment(num_envs, device="cuda:0", max_episode_steps=1000, warmstart=0.0, push_force=0.0, push_interval=100,
                      push_duration=5, push_probability=1.0, seed=0, control_mode=None, variable_stiffness=False,
                      gain_scale=0.0, terminate=None, observations=None, rewards=None, command=None, motion=None, sensing=None,
                      randomize=None, monitor=None, critic=None, start_state=None):   # (weights of trex_train.py:66)
    # control_mode: what the joints' actions mean (position / velocity / torque: J-wide, through the trainer unchanged). The
    # 2J-wide stiffness action space is wider than the policy kernel's act_dim <= 32: refused here, not deep in a launch
    check_action_space(control_mode, variable_stiffness)
    # warmstart > 0: the contact solver starts from that fraction of each point's impulses of the last solve (model parameter)
    params = {"warmstart": float(warmstart)} if warmstart else None
    # push_force > 0: random horizontal pushes of the base, up to push_force N, every push_interval env-steps for
    # push_duration env-steps (trex_gym.perturb.RandomPushes); 0 = none
    # observations: a preset's name ("locomotion") or a specification of trex_gym.observations (a checkpoint's): extra
    # observation columns composed on the device; None = the reference's 3J columns
    if isinstance(observations, str):
        from . import _capi, observations as O
        if observations not in O.PRESETS:
            raise ValueError("--observations: expected one of %s, got %r" % (", ".join(sorted(O.PRESETS)), observations))
        observations = O.PRESETS[observations](_capi.Model(_URDF_PATH), device)
    elif observations is not None:
        from . import observations as O
        observations = O.from_tuples(observations)
    # rewards: a preset's name ("locomotion") or a specification of trex_gym.rewards (a checkpoint's): the reward column composed
    # on the device from its terms; command: (vx, vy, yaw rate) for every env, and - with observations - three more observation
    # columns, so that the policy sees what it is rewarded for; None = the step's own reward
    if isinstance(rewards, str):
        from . import _capi, rewards as R
        if rewards not in R.PRESETS:
            raise ValueError("--rewards: expected one of %s, got %r" % (", ".join(sorted(R.PRESETS)), rewards))
        rewards = R.PRESETS[rewards](_capi.Model(_URDF_PATH), device)
    elif rewards is not None:
        from . import rewards as R
        rewards = R.from_tuples(rewards)
    # motion: dict(clip=path of a Clip.save() file, rsi=, weight=, terms=) - a reference motion on the device, its tracking terms
    # (trex_gym.motion.imitation, their weights times `weight`; or a checkpoint's) added to the reward column, with rsi every new
    # episode started at a random instant of the clip, and - with observations - sin and cos of the clip's phase as two more
    # observation columns behind the commands'
    external = None
    command_columns = rewards is not None and observations is not None
    phase_columns = motion is not None and observations is not None
    if command_columns or phase_columns:
        from . import motion as M, observations as O
        observations = list(observations) + (O.external(3) if command_columns else []) + (O.external(2) if phase_columns else [])
        if command_columns and phase_columns:
            external = lambda env: torch.cat([env.commands, M.phase_columns(env)], 1)
        else:
            external = (lambda env: env.commands) if command_columns else M.phase_columns
    pushes = None
    if push_force > 0:
        dev = torch.device(device)
        gen = torch.Generator(device=dev).manual_seed(int(seed))
        pushes = RandomPushes(num_envs, body=0, interval=push_interval, probability=push_probability, max_force=push_force,
                              duration=push_duration, generator=gen, device=dev)
    env = TrexVecEnv(num_envs, urdf_path=_URDF_PATH, device=device, distance_weight=2e2, energy_weight=1e-6,
                     drift_weight=1.0, max_episode_steps=max_episode_steps, params=params, pushes=pushes, control_mode=control_mode,
                     terminate=terminate, observations=observations, external=external, rewards=rewards)   # terminate: TrexVecEnv.set_termination's arguments - a fall ends the episode, on the device
    env.command_columns = command_columns   # the last channel is the commands': a checkpoint stores the channels without it
    env.phase_columns = phase_columns       # and behind it the phase's, likewise
    env.motion_config = None
    if motion is not None:
        from . import motion as M
        from .termination import foot_links
        weight = float(motion.get("weight", 1.0))
        feet = [(l, (0.0, 0.0, 0.0)) for l in foot_links(env)][:M.MAX_END_EFFECTORS]
        terms = M.imitation(env.model, end_effectors=bool(feet)) if motion.get("terms") is None else M.from_tuples(motion["terms"])
        if motion.get("terms") is None:
            terms = [t._replace(weight=t.weight * weight) for t in terms]
        clip = motion["clip"]
        if motion.get("mirror_clip"):       # the clip and its mirror image, one behind the other (trex_gym.symmetry.clip_with_mirror)
            from .symmetry import Mirror, clip_with_mirror
            clip = clip_with_mirror(M.Clip.load(clip), Mirror(env, log=None))
        M.attach(env, clip, terms=terms, end_effectors=feet, rsi=bool(motion.get("rsi", False)), seed=seed)
        # what a checkpoint stores: the clip's path, the terms as set (the weight is in them), the rsi and mirror flags
        env.motion_config = dict(clip=str(motion["clip"]), rsi=bool(motion.get("rsi", False)), weight=1.0, terms=M.as_tuples(terms),
                                 mirror_clip=bool(motion.get("mirror_clip", False)))
    # sensing: dict(preset="typical" or None, scale=, obs_delay=(min, max), action_delay=(min, max)) as the flags give it, or
    # dict(groups=, action_delay=, seed=) - a checkpoint's, the recorded specification of trex_gym.sensing.attach: the policy reads
    # its observations through sensors (noise, bias, resolution, latency, on the device) and its actions reach the motors late
    env.sensing_config = None
    if sensing is not None:
        from . import sensing as S
        if "groups" in sensing:
            spec, sense_seed = S.from_tuples(sensing["groups"]), sensing.get("seed", seed)
        else:
            sense_seed, delay = seed, tuple(sensing.get("obs_delay") or (0, 0))
            if sensing.get("preset") is not None:
                if sensing["preset"] not in S.PRESETS:
                    raise ValueError("--sensing: expected one of %s, got %r" % (", ".join(sorted(S.PRESETS)), sensing["preset"]))
                spec = S.PRESETS[sensing["preset"]](env, scale=float(sensing.get("scale", 1.0)), delay=delay)
            else:   # (a latency alone: on q, qd and every channel the env composes itself)
                spec = S.latency([(0, 2 * env.J)] + ([(3 * env.J, env.obs_dim - 3 * env.J)] if env.obs_dim > 3 * env.J else []), delay) \
                    if delay[1] > 0 else []
        S.attach(env, spec, action_delay=tuple(sensing.get("action_delay") or (0, 0)), seed=sense_seed)
        env.sensing_config = env.sensing     # what a checkpoint stores: the groups as set, the action delay, the seed
    if command is not None:
        if rewards is None:
            raise ValueError("--command: there are no reward terms to track it (--rewards)")
        env.commands[:] = torch.tensor([float(x) for x in command], device=env.device)
    env.command = None if command is None else [float(x) for x in command]
    # randomize: dict(preset="typical", scale=, push=, command_range=, command_interval=) as the flags give it, or dict(terms=, seed=)
    # - a checkpoint's, the recorded specification of trex_gym.randomize.attach: mass scale, friction, motor gains, pushes and the
    # command redrawn on the device when an episode starts or at an interval inside it (behind --command: the terms overwrite it)
    env.randomize_config = None
    if randomize is not None:
        from . import randomize as Z
        if "terms" in randomize:
            spec, rand_seed = Z.from_tuples(randomize["terms"]), randomize.get("seed", seed)
        else:
            if randomize.get("preset") not in Z.PRESETS:
                raise ValueError("--randomize: expected one of %s, got %r" % (", ".join(sorted(Z.PRESETS)), randomize.get("preset")))
            kw = {}
            if randomize.get("push") is not None:
                kw["push_force"] = float(randomize["push"])
            if randomize.get("command_interval") is not None:
                kw["command_interval"] = int(randomize["command_interval"])
            if randomize.get("command_range") is not None:
                kw["command_range"] = tuple(float(x) for x in randomize["command_range"])
            spec, rand_seed = Z.PRESETS[randomize["preset"]](env, scale=float(randomize.get("scale", 1.0)), **kw), seed
        Z.attach(env, spec, seed=rand_seed)
        env.randomize_config = env.randomization     # what a checkpoint stores: the terms as set, the seed
    # start_state: dict(preset="typical", scale=, clearance=(lo, hi) or None) as the flags give it, or dict(terms=, seed=) - a
    # checkpoint's, the recorded specification of trex_gym.start_state.attach: the state an episode starts in - joint angles and
    # velocities, base attitude and velocity - perturbed on the device, on top of the reset's or RSI's state, and placed on the floor
    env.start_state_config = None
    if start_state is not None:
        from . import start_state as SS
        if "terms" in start_state:
            spec, start_seed = SS.from_tuples(start_state["terms"]), start_state.get("seed", seed)
        else:
            if start_state.get("preset") not in SS.PRESETS:
                raise ValueError("--start_noise: expected one of %s, got %r" % (", ".join(sorted(SS.PRESETS)), start_state.get("preset")))
            clearance = start_state.get("clearance")
            spec = SS.PRESETS[start_state["preset"]](env, scale=float(start_state.get("scale", 1.0)),
                                                     clearance=None if clearance is None else tuple(float(x) for x in clearance))
            start_seed = seed
        SS.attach(env, spec, seed=start_seed)
        env.start_state_config = env.start_state     # what a checkpoint stores: the terms as set, the seed
    if gain_scale > 0:   # every episode with motor gains and strength scaled by 1 +- gain_scale per env (RandomGains)
        dev = torch.device(device)
        r = (1.0 - gain_scale, 1.0 + gain_scale)
        env.gains = RandomGains(env.num_envs, env.J, kp_scale=r, kd_scale=r, max_force_scale=r,
                                generator=torch.Generator(device=dev).manual_seed(int(seed) + 1), device=dev)
    # monitor: dict(window=, terms=) - the flag's, or a checkpoint's: the episode monitor of trex_gym.monitor.attach, behind the
    # rewards and the motion clip, whose term blocks it sums per episode
    env.monitor_config = None
    if monitor is not None:
        from . import monitor as monitoring
        monitoring.attach(env, window=int(monitor.get("window", 100)), terms=bool(monitor.get("terms", True)))
        env.monitor_config = env.monitor             # what a checkpoint stores: settings only
    # critic: a preset's name of trex_gym.critic ("clean", "privileged"): the row the value net of an asymmetric actor-critic reads,
    # attached last - behind the sensor model and the randomisation whose draws it reads
    env.critic_config = None
    if critic is not None:
        from . import critic as critics
        if critic not in critics.PRESETS:
            raise ValueError("--critic: expected one of %s, got %r" % (", ".join(sorted(critics.PRESETS)), critic))
        critics.PRESETS[critic](env)
        env.critic_config = dict(preset=critic, spec=env.critic_spec, names=list(env.critic_names))    # what a checkpoint stores
    return env


POLICY_MAX_ACT_DIM = 32      # the policy kernel's widest action (csrc/policy_limits.h)


def check_action_space(control_mode, variable_stiffness, num_joints=25):
    if control_mode is not None and not isinstance(control_mode, (dict, list, tuple)) and control_mode not in actuators.CONTROL_MODES:
        raise ValueError("--control_mode: expected one of %s, got %r" % (", ".join(actuators.CONTROL_MODES), control_mode))
    if variable_stiffness and 2 * num_joints > POLICY_MAX_ACT_DIM:
        raise ValueError("variable stiffness makes the action space %d wide; the policy kernel takes at most %d: "
                         "not supported by this trainer" % (2 * num_joints, POLICY_MAX_ACT_DIM))


# Hyper-parameter presets. "reference" is the ppo2.learn call of the reference's script (trex_train.py:47-60):
# noptepochs 32, nminibatches 32, lam 0.95, gamma 0.99, lr 3e-4, cliprange 0.2, ent_coef 0. Its rollout is
# nsteps = 4096 samples of ONE env per update; here an update takes nsteps x num_envs samples of the batched env
# (nsteps 32 by default: 131072 samples at 4096 envs, minibatches of 4096). "throughput" is the same except 4 epochs
# per update - what the bench-style measurements of config 3 use.
PRESETS = {
    "reference": dict(nminibatches=32, noptepochs=32, lam=0.95, gamma=0.99, lr=3e-4, cliprange=0.2, ent_coef=0.0),
    "throughput": dict(nminibatches=32, noptepochs=4, lam=0.95, gamma=0.99, lr=3e-4, cliprange=0.2, ent_coef=0.0),
}


def train(env, num_timesteps, seed, nsteps=32, noptepochs=None, save_path=None, log=print, use_graphs=False,
          preset="throughput", distill=None, symmetry=None, sym_coef=1.0):
    """distill: dict(teacher=PATH, rows="clean" | "critic" | "rows", loss="kl" | "mse", beta=, decay=) - the student of
    trex_gym.distill.Distill is trained onto that teacher instead of PPO on the reward (the preset's nminibatches, noptepochs and lr
    hold); the checkpoint is an ordinary one and records the teacher's path and row choice.
    symmetry: "augment", "loss" or "both" trains trex_gym.symmetry.MirrorPPO - on every rollout sample and its mirror image, with
    the mirror loss weighted sym_coef, or both -; the mirror tables and the option travel in the checkpoint."""
    hp = dict(PRESETS[preset])
    if noptepochs is not None:
        hp["noptepochs"] = noptepochs
    if distill is not None:
        from .distill import Distill, Teacher
        teacher = Teacher(env, distill["teacher"], rows=distill.get("rows", "clean"))
        agent = Distill(env, teacher, nsteps=nsteps, nminibatches=hp["nminibatches"], noptepochs=hp["noptepochs"], lr=hp["lr"],
                        loss=distill.get("loss", "kl"), beta=float(distill.get("beta", 1.0)), beta_decay=float(distill.get("decay", 0.9)),
                        seed=seed, use_graphs=use_graphs)
    elif symmetry is not None:
        from .symmetry import Mirror, MirrorPPO
        if getattr(env, "critic_config", None) is not None:
            raise ValueError("--symmetry is not written for --critic")
        agent = MirrorPPO(env, Mirror(env, log=log), symmetry=symmetry, sym_coef=sym_coef, nsteps=nsteps, seed=seed,
                          use_graphs=use_graphs, **hp)
    else:
        agent = PPO(env, nsteps=nsteps, seed=seed, use_graphs=use_graphs, critic=getattr(env, "critic_config", None) is not None, **hp)
    log("Number of actions: %d; number of joints: %d; model mass: %.2f; nsteps %d x %d envs; preset %s, noptepochs %d"
        % (env.action_space.shape[0], env.model.num_joints, env.model.total_mass(False), nsteps, env.num_envs, preset,
           hp["noptepochs"]))
    hist = agent.learn(num_timesteps, log=log)
    if save_path:
        st = agent.kern.get_stats()     # VecNormalize's running statistics travel with the weights (trex_train.py:93-99 restores both)
        torch.save({"theta": agent.policy.theta.detach().clone(), "obs_mean": torch.tensor(st["obs_mean"]),
                    "obs_var": torch.tensor(st["obs_var"]), "obs_count": torch.tensor(float(st["obs_count"])),
                    "ret_var": torch.tensor(float(st["ret_var"])),
                    "observations": _own_channels(env), "rewards": getattr(env, "rewards", None),
                    "command": getattr(env, "command", None), "motion": getattr(env, "motion_config", None),
                    "sensing": getattr(env, "sensing_config", None), "randomize": getattr(env, "randomize_config", None),
                    "start_state": getattr(env, "start_state_config", None),
                    "monitor": getattr(env, "monitor_config", None), "critic": critic_checkpoint(agent),
                    "distill": None if distill is None else dict(teacher=str(distill["teacher"]), rows=str(distill.get("rows", "clean")),
                                                                 loss=str(distill.get("loss", "kl"))),
                    "symmetry": None if getattr(agent, "mirror", None) is None else dict(mode=agent.symmetry, sym_coef=float(agent.sym_coef),
                                                                                         **agent.mirror.tables())},
                   save_path)   # (the channels, the terms, the clip and the sensor model: --play rebuilds the same row)
    return agent, hist


def critic_checkpoint(agent):
    """what a checkpoint stores of a privileged critic - None without one: the width (theta's vf.W1 has that many rows), the
    recorded sources and column names, and the critic's running moments. Playing needs the width alone."""
    if getattr(agent, "crit", None) is None:
        return None
    st = agent.crit.get_stats()
    cfg = getattr(agent.env, "critic_config", None) or dict(preset=None, spec=getattr(agent.env, "critic_spec", None),
                                                            names=list(getattr(agent.env, "critic_names", [])))
    return dict(dim=int(agent.critic_dim), preset=cfg["preset"], spec=cfg["spec"], names=cfg["names"],
                mean=torch.tensor(st["mean"]), var=torch.tensor(st["var"]), count=torch.tensor(float(st["count"]), dtype=torch.float64))


def _own_channels(env):
    """the env's observation channels as a checkpoint stores them: without the three command columns and the two phase columns
    build_environment adds behind them when rewards or a motion clip are set (env.command_columns and env.phase_columns say
    that it did) (it adds them again on loading)"""
    obs = getattr(env, "observations", None)
    added = int(getattr(env, "command_columns", False)) + int(getattr(env, "phase_columns", False))
    if obs is not None and added:
        obs = obs[:-added]
    return obs


def _png_writer():
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("play(frames_dir=...) writes PNGs with Pillow (PIL), which is not installed") from e
    return Image


def play(agent, num_play_timesteps, export_path=None, env_index=0, log=print, deterministic=False, update_stats=True, seed=0,
         frames_dir=None, frame_size=(960, 720), camera=None, symmetric=False):
    """The reference's play loop (trex_train.py:126-136: model.step -> env.step -> render a frame -> PNGs -> ffmpeg) up to
    the movie: every frame's world poses of the 252 visual meshes are recorded (trex_batch_visual_transforms) - what an
    external mesh renderer needs -, and with frames_dir a PNG of the collision hulls is written per step.
    Defaults = the reference's behaviour: `model.step(obs)[0]` is a SAMPLED action (deterministic=False: N(0, 1) noise for
    the policy kernel) and the VecNormalize env it plays in keeps updating its running statistics with every observation
    (update_stats=True: the statistics kernel runs after each step). deterministic=True plays the mean action,
    update_stats=False freezes the statistics after the reset - the repeatable variant for comparing checkpoints (what this
    function did until round 3, then under the name of the reference's loop).
    export_path: .npz with `mesh_files`, `mesh_links`, `poses` [T, 252, 7] (xyz + quaternion xyzw of env `env_index`),
    `reward` [T], `fps` = 50 (metadata of trex_env.py:36).
    frames_dir: one PNG per step of env `env_index` ('%05d-of-%05d.png', the reference's names), frame_size = (width,
    height), camera = trex_gym.render.Camera (default: the reference's, following the base)."""
    import numpy as np
    env, k = agent.env, agent.kern
    noise = torch.zeros(env.num_envs, env.J, device=env.device)
    gen = torch.Generator(device=env.device).manual_seed(int(seed))
    frames, rewards = [], []
    if frames_dir is not None:
        Image = _png_writer()
        os.makedirs(frames_dir, exist_ok=True)
    mirror = None
    if symmetric:       # (the mean action made mirror-equivariant: trex_gym.symmetry.Mirror.symmetric_action; no noise is drawn)
        from .symmetry import Mirror
        mirror = getattr(agent, "mirror", None) or Mirror(env, log=log)
    env.reset_tensor()
    k.observe(env.rows, with_reward=False)
    for _ in range(num_play_timesteps):
        if not deterministic:
            noise.normal_(generator=gen)
        if mirror is not None:
            mirror.symmetric_action(agent, out=agent.actions)
        elif getattr(agent, "crit", None) is not None:    # (trained with a privileged critic: the policy alone, no critic row)
            agent.crit.act(agent.policy.theta, env.rows, None, noise, agent.actions, clip_obs=agent.clip_obs)
        else:
            k.act(agent.policy.theta, env.rows, noise, agent.actions, clip_obs=agent.clip_obs)
        env.step_tensor(agent.actions)
        if update_stats:
            k.observe(env.rows)       # (VecNormalize.step_wait: the observation moments AND the return moments move on)
        frames.append(env.visual_transforms()[env_index].cpu().numpy())
        rewards.append(float(env.rew[env_index]))
        if frames_dir is not None:
            rgb = env.render_tensor([env_index], frame_size[0], frame_size[1], camera)[0].cpu().numpy()
            Image.fromarray(rgb).save(os.path.join(frames_dir, "%05d-of-%05d.png" % (len(rewards) - 1, num_play_timesteps)))
    log("Episode reward: %.3f over %d frames" % (sum(rewards), len(rewards)))
    if getattr(env, "monitor_api", None) is not None:   # (the episode monitor's view: the last episode the env finished)
        from . import monitor as monitoring
        last = monitoring.last_episode(env)
        log("Last finished episode: return %.3f, length %d, end reason %d; %d finished; running: return %.3f, length %d"
            % (float(last["return"][env_index]), int(last["length"][env_index]), int(last["reason"][env_index]),
               int(last["episodes"][env_index]), float(last["running_return"][env_index]), int(last["running_length"][env_index])))
    if export_path:
        table = env.model.visuals()
        np.savez_compressed(export_path, mesh_files=np.array([t[0] for t in table]), mesh_links=np.array([t[1] for t in table]),
                            poses=np.stack(frames).astype(np.float32), reward=np.array(rewards, np.float32), fps=np.float32(50.0))
    return np.stack(frames), np.array(rewards)


def load_agent(load_path, num_envs=1, device="cuda:0", max_episode_steps=1000, sensing=True, randomize=True, start_state=True):
    """trex_train.py:75-110 (replay): rebuild the policy from a file written by train(save_path=...) - the flat
    parameter vector and VecNormalize's statistics. sensing=False: without the sensor model the checkpoint was trained with; randomize=False:
    without its episode randomisation; start_state=False: without its start-state randomisation."""
    ck = torch.load(load_path, map_location=device, weights_only=True)
    env = build_environment(num_envs, device=device, max_episode_steps=max_episode_steps, observations=ck.get("observations"),
                            rewards=ck.get("rewards"), command=ck.get("command"), motion=ck.get("motion"),
                            sensing=ck.get("sensing") if sensing else None, randomize=ck.get("randomize") if randomize else None,
                            monitor=ck.get("monitor"), start_state=ck.get("start_state") if start_state else None)
    agent = PPO(env, nsteps=1, nminibatches=1, noptepochs=1)
    cr = ck.get("critic")
    if cr is not None:      # theta has the critic's layout; the env gets no critic row: playing runs the policy alone
        from . import critic_capi
        from .ppo import MlpPolicy
        agent.crit, agent.critic_dim = critic_capi.PolicyCritic(agent.kern), int(cr["dim"])
        agent.crit.set(agent.critic_dim)
        agent.crit.set_stats(dict(mean=cr["mean"].cpu().numpy(), var=cr["var"].cpu().numpy(), count=float(cr["count"])))
        agent.policy = MlpPolicy(agent.crit.layout, agent.crit.param_count, agent.dev)
        agent.critic_config = {k: cr[k] for k in ("preset", "spec", "names")}
    with torch.no_grad():
        agent.policy.theta.copy_(ck["theta"])
    st = agent.kern.get_stats()
    st.update(obs_mean=ck["obs_mean"].cpu().numpy(), obs_var=ck["obs_var"].cpu().numpy(), obs_count=float(ck["obs_count"]),
              ret_var=float(ck["ret_var"]))
    agent.kern.set_stats(st)
    return agent


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true", default=True)
    ap.add_argument("--num_timesteps", type=int, default=int(5e6))   # trex_train.py:27
    ap.add_argument("--random_seed", type=int, default=0)            # trex_train.py:29
    ap.add_argument("--num_envs", type=int, default=4096)
    ap.add_argument("--nsteps", type=int, default=32)
    ap.add_argument("--preset", choices=sorted(PRESETS), default="reference",
                    help="reference: the hyper-parameters of the reference's ppo2.learn call (32 epochs per update)")
    ap.add_argument("--noptepochs", type=int, default=None, help="override the preset's epochs per update")
    ap.add_argument("--max_episode_steps", type=int, default=1000)
    ap.add_argument("--save", type=str, default=None)
    ap.add_argument("--warmstart", type=float, default=0.0,
                    help="PGS warm start: contact points start each solve at this factor x their last impulses, in [0, 1] (0 = off)")
    ap.add_argument("--graphs", action="store_true", help="replay the rollout and the minibatch update as HIP graphs")
    ap.add_argument("--play", action="store_true", help="after training: run the policy and record the frames' mesh poses (trex_train.py:25,126-136)")
    ap.add_argument("--num_play_timesteps", type=int, default=int(2e3))          # trex_train.py:28
    ap.add_argument("--export", type=str, default=None, help="with --play: .npz of mesh names + [T, 252, 7] world poses for an external renderer")
    ap.add_argument("--frames", type=str, default=None, help="with --play: directory for one 960 x 720 PNG per step (trex_train.py:132-134)")
    ap.add_argument("--play_deterministic", action="store_true", help="with --play: the mean action and frozen normalisation statistics (the reference samples and keeps updating)")
    ap.add_argument("--push_force", type=float, default=0.0,
                    help="random horizontal pushes of the base of up to this many N (0 = off; trex_gym.perturb.RandomPushes)")
    ap.add_argument("--push_interval", type=int, default=100, help="with --push_force: env-steps between two pushes of an env")
    ap.add_argument("--push_duration", type=int, default=5, help="with --push_force: env-steps a push lasts")
    ap.add_argument("--control_mode", choices=sorted(actuators.CONTROL_MODES), default="position",
                    help="what an action is for every joint: target angle, target velocity or torque")
    ap.add_argument("--variable_stiffness", action="store_true", help="[target, stiffness] actions (2J wide): refused, wider than the policy kernel")
    ap.add_argument("--gain_scale", type=float, default=0.0, help="randomise motor kp / kd / max_force per env and episode by 1 +- this (0 = off)")
    ap.add_argument("--terminate_head_height", type=float, default=None, help="end an episode when the head is lower than this above the floor (m)")
    ap.add_argument("--terminate_tilt", type=float, default=None, help="end an episode when the base is tipped more than this from its start orientation (rad)")
    ap.add_argument("--terminate_contact", type=str, default=None, metavar="LINK[,LINK...]",
                    help="end an episode when one of these links touches the floor; 'auto': every body but the feet of the start pose")
    ap.add_argument("--observations", choices=["locomotion"], default=None,
                    help="extra observation columns composed on the device; locomotion: base tilt, velocity, height, the feet's contact "
                         "force and position (18 columns; default: the reference's 75 alone)")
    ap.add_argument("--rewards", choices=["locomotion"], default=None,
                    help="reward terms composed on the device; locomotion: velocity tracking, a quiet upright base, small torques, "
                         "smooth actions, swinging feet that do not slide, nothing but the feet on the floor (default: the step's reward)")
    ap.add_argument("--command", type=float, nargs=3, default=None, metavar=("VX", "VY", "WZ"),
                    help="with --rewards: the velocity every env is to track - forward, sideways (m/s, base axes), yaw rate (rad/s)")
    ap.add_argument("--motion", type=str, default=None, metavar="CLIP.npz",
                    help="a reference motion (trex_gym.motion.Clip.save): DeepMimic's tracking terms against it are added to the reward on "
                         "the device; with --observations, sin and cos of the clip's phase join the observation (with --observations "
                         "locomotion and --rewards that is 93 + 3 + 2 = 98 columns, more than the learner's 96: not supported)")
    ap.add_argument("--mirror_clip", action="store_true",
                    help="with --motion: train on the clip and its mirror image, one behind the other (trex_gym.symmetry.clip_with_mirror)")
    ap.add_argument("--rsi", action="store_true", help="with --motion: every new episode starts at a random instant of the clip")
    ap.add_argument("--motion_weight", type=float, default=1.0, help="with --motion: a factor on the weights of the tracking terms")
    ap.add_argument("--sensing", choices=["typical"], default=None,
                    help="the policy reads its observations through sensors, on the device; typical: white noise on q, qd, the base's "
                         "tilt, velocities and height, a bias per episode on q, tilt and gyro, a 12-bit encoder (trex_gym.sensing.typical)")
    ap.add_argument("--sense_scale", type=float, default=1.0, help="with --sensing: a factor on the preset's noise and bias")
    ap.add_argument("--obs_delay", type=int, nargs=2, default=None, metavar=("MIN", "MAX"),
                    help="sensing latency in env-steps, drawn per env and episode in [MIN, MAX] (at most 8)")
    ap.add_argument("--action_delay", type=int, nargs=2, default=None, metavar=("MIN", "MAX"),
                    help="actuation latency in env-steps, drawn per env and episode in [MIN, MAX] (at most 8)")
    ap.add_argument("--no_sensing", action="store_true", help="with --play: run the policy without the sensor model it was trained with")
    ap.add_argument("--randomize", choices=["typical"], default=None,
                    help="episode randomisation on the device, redrawn whenever an episode starts: typical: mass scale, friction, "
                         "motor gains, a push of the base and - with --rewards - the command (trex_gym.randomize.typical)")
    ap.add_argument("--rand_scale", type=float, default=1.0, help="with --randomize: a factor on the width of the preset's ranges")
    ap.add_argument("--rand_push", type=float, default=None, metavar="N",
                    help="with --randomize: the largest push in newtons; 0 drops the preset's push term")
    ap.add_argument("--command_range", type=float, nargs=3, default=None, metavar=("VX", "VY", "WZ"),
                    help="with --randomize: the half-widths the command's components are drawn in")
    ap.add_argument("--command_interval", type=int, default=None, metavar="K",
                    help="with --randomize: env-steps between two draws of the command inside an episode (0: per episode only)")
    ap.add_argument("--monitor", type=int, nargs="?", const=100, default=None, metavar="WINDOW",
                    help="episode monitor on the device: eprewmean, eplenmean and the end reasons of the last WINDOW (100) finished "
                         "episodes per iteration (trex_gym.monitor)")
    ap.add_argument("--no_randomize", action="store_true", help="with --play: run the policy without the episode randomisation it was trained with")
    ap.add_argument("--start_noise", choices=["typical"], default=None,
                    help="start-state randomisation on the device, on top of the reset's or --rsi's state: typical: joint angles and "
                         "velocities, roll, pitch, yaw, base velocities - untuned magnitudes (trex_gym.start_state.typical)")
    ap.add_argument("--start_scale", type=float, default=1.0, help="with --start_noise: a factor on the width of the preset's ranges")
    ap.add_argument("--start_clearance", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="with --start_noise: place the perturbed robot with its lowest collision point LO..HI metres above the floor")
    ap.add_argument("--no_start_noise", action="store_true", help="with --play: run the policy without the start-state randomisation it was trained with")
    ap.add_argument("--fall_penalty", type=float, default=0.0, help="taken from the reward of the step in which an episode ends by a fall")
    ap.add_argument("--symmetry", choices=["augment", "loss", "both"], default=None,
                    help="train on every rollout sample and its mirror image, with a mirror loss on the policy mean, or both "
                         "(trex_gym.symmetry.MirrorPPO; include/trex_symmetry.h)")
    ap.add_argument("--sym_coef", type=float, default=1.0, help="with --symmetry loss | both: the weight of the mirror loss")
    ap.add_argument("--symmetric", action="store_true",
                    help="with --play: step the env with (mu(s) + M_a mu(M_o s)) / 2, the mean action made mirror-equivariant")
    ap.add_argument("--critic", choices=["clean", "privileged"], default=None,
                    help="asymmetric actor-critic: the value net reads a row of its own - the observation before the sensor model "
                         "(clean), plus friction, push force, mass scale and foot contact forces where the env has them (privileged) - "
                         "during training only (trex_gym.critic)")
    ap.add_argument("--distill", type=str, default=None, metavar="TEACHER.ckpt",
                    help="policy distillation: regress the student, which reads the env's (sensor) row, onto this trained teacher "
                         "instead of running PPO on the reward (trex_gym.distill)")
    ap.add_argument("--teacher_rows", choices=["clean", "critic", "rows"], default="clean",
                    help="with --distill: what the teacher reads - the row before the sensor model, the critic row (--critic), the env's row")
    ap.add_argument("--distill_loss", choices=["kl", "mse"], default="kl",
                    help="with --distill: KL(teacher || student) of the action distributions, or half the squared error of the means")
    ap.add_argument("--dagger_beta", type=float, nargs="+", default=None, metavar=("B", "DECAY"),
                    help="with --distill: the probability B that an env follows the teacher during a rollout (default 1), "
                         "multiplied by DECAY (default 0.9) after every rollout")
    ap.add_argument("--mpc", type=int, nargs=2, default=None, metavar=("SAMPLES", "HORIZON"),
                    help="no training: control the envs with the sampling-based planner (trex_gym.planner) - SAMPLES rollouts of "
                         "HORIZON steps per env and control step; --graphs replays a planning iteration, --frames writes PNGs")
    ap.add_argument("--mpc_knots", type=int, default=None, metavar="P", help="with --mpc: spline knots of an action sequence (default min(HORIZON, 6))")
    ap.add_argument("--mpc_sigma", type=float, default=None, metavar="X", help="with --mpc: the standard deviation of a knot's noise (default 0.1)")
    ap.add_argument("--mpc_temperature", type=float, default=None, metavar="L",
                    help="with --mpc: the temperature of the return weighting; 0 keeps the best sample alone (default 0.1)")
    ap.add_argument("--mpc_iterations", type=int, default=None, metavar="I", help="with --mpc: sample - rollout - update rounds per control step (default 1)")
    ap.add_argument("--mpc_steps", type=int, default=None, metavar="T", help="with --mpc: control steps to run (default 100)")
    ap.add_argument("--save_clip", type=str, default=None, metavar="FILE.npz",
                    help="with --mpc: the states the envs went through, [T, N, state width] with the frame time, for motion.Clip.from_states")
    args = ap.parse_args(argv)
    mpc_flags = ("mpc_knots", "mpc_sigma", "mpc_temperature", "mpc_iterations", "mpc_steps", "save_clip")
    if args.mpc is None and any(getattr(args, f) is not None for f in mpc_flags):
        ap.error("--mpc_knots, --mpc_sigma, --mpc_temperature, --mpc_iterations, --mpc_steps and --save_clip need --mpc")
    if args.mpc is not None:
        if args.save is not None or args.play or args.export is not None or args.distill is not None or args.critic is not None \
                or args.noptepochs is not None or args.preset != "reference":
            ap.error("--mpc plans and does not train: not with --save, --play, --export, --distill, --critic, --noptepochs or --preset")
        if not (1 <= args.mpc[0] <= 4096 and 1 <= args.mpc[1] <= 256):
            ap.error("--mpc: 1 <= SAMPLES <= 4096, 1 <= HORIZON <= 256")
        if args.mpc_knots is not None and not 1 <= args.mpc_knots <= min(args.mpc[1], 32):
            ap.error("--mpc_knots: 1 <= P <= min(HORIZON, 32)")
        if (args.mpc_sigma is not None and not (args.mpc_sigma >= 0.0 and math.isfinite(args.mpc_sigma))) or \
                (args.mpc_temperature is not None and not (args.mpc_temperature >= 0.0 and math.isfinite(args.mpc_temperature))):
            ap.error("--mpc_sigma and --mpc_temperature must be finite and not negative")
        if (args.mpc_iterations is not None and args.mpc_iterations < 1) or (args.mpc_steps is not None and args.mpc_steps < 1):
            ap.error("--mpc_iterations and --mpc_steps: at least 1")
    if args.distill is None and (args.teacher_rows != "clean" or args.distill_loss != "kl" or args.dagger_beta is not None):
        ap.error("--teacher_rows, --distill_loss and --dagger_beta need --distill")
    if args.dagger_beta is not None and (len(args.dagger_beta) > 2 or not all(0.0 <= x <= 1.0 for x in args.dagger_beta)):
        ap.error("--dagger_beta: B [DECAY], both in [0, 1]")
    if args.distill is not None and args.teacher_rows == "critic" and args.critic is None:
        ap.error("--teacher_rows critic needs --critic (the row the teacher reads)")
    if args.variable_stiffness:
        try:
            check_action_space(args.control_mode, True)
        except ValueError as e:
            ap.error(str(e))
    if args.command is not None and args.rewards is None:
        ap.error("--command needs --rewards")
    if args.motion is None and (args.rsi or args.motion_weight != 1.0 or args.mirror_clip):
        ap.error("--rsi, --mirror_clip and --motion_weight need --motion")
    if args.rsi and args.graphs:   # (the instants are drawn per step by a generator of the env's own: not in a replayed graph)
        ap.error("--rsi cannot be combined with --graphs")
    if args.sensing is None and args.sense_scale != 1.0:
        ap.error("--sense_scale needs --sensing")
    if not (args.sense_scale >= 0.0):
        ap.error("--sense_scale must not be negative")
    for name in ("obs_delay", "action_delay"):
        d = getattr(args, name)
        if d is not None and not 0 <= d[0] <= d[1] <= 8:
            ap.error("--%s: 0 <= MIN <= MAX <= 8" % name)
    if args.monitor is not None and not 1 <= args.monitor <= 65536:
        ap.error("--monitor: a window of 1 to 65536 episodes")
    if args.randomize is None and (args.rand_scale != 1.0 or args.rand_push is not None or args.command_range is not None
                                   or args.command_interval is not None):
        ap.error("--rand_scale, --rand_push, --command_range and --command_interval need --randomize")
    if not (args.rand_scale >= 0.0) or (args.rand_push is not None and not args.rand_push >= 0.0):
        ap.error("--rand_scale and --rand_push must not be negative")
    if args.command_range is not None and not all(x >= 0.0 for x in args.command_range):
        ap.error("--command_range: half-widths must not be negative")
    if args.command_interval is not None and args.command_interval < 0:
        ap.error("--command_interval must not be negative")
    if args.start_noise is None and (args.start_scale != 1.0 or args.start_clearance is not None):
        ap.error("--start_scale and --start_clearance need --start_noise")
    if not (args.start_scale >= 0.0):
        ap.error("--start_scale must not be negative")
    if args.start_clearance is not None and not (math.isfinite(args.start_clearance[0]) and args.start_clearance[0] <= args.start_clearance[1]
                                                 and math.isfinite(args.start_clearance[1])):
        ap.error("--start_clearance: LO <= HI, both finite")
    if args.randomize is not None and (args.push_force > 0 or args.gain_scale > 0):   # (one owner per buffer)
        ap.error("--randomize cannot be combined with --push_force or --gain_scale")
    if not 0.0 <= args.gain_scale < 1.0:
        ap.error("--gain_scale must lie in [0, 1)")
    if args.push_force > 0 and args.graphs:   # (the pushes are drawn per step on the host's step count: not in a replayed graph)
        ap.error("--push_force cannot be combined with --graphs")
    if args.gain_scale > 0 and args.graphs and termination_args(args):   # (a fallen env draws new gains: host work per step)
        ap.error("--gain_scale with a --terminate_* criterion cannot be combined with --graphs")
    return args


def sensing_args(args):
    """the dict for build_environment(sensing=...) of the --sensing, --sense_scale, --obs_delay and --action_delay flags, None when
    none is given"""
    if args.sensing is None and args.obs_delay is None and args.action_delay is None:
        return None
    return dict(preset=args.sensing, scale=args.sense_scale, obs_delay=args.obs_delay, action_delay=args.action_delay)


def monitor_args(args):
    """the dict for build_environment(monitor=...) of the --monitor flag, None when it is not given"""
    if args.monitor is None:
        return None
    return dict(window=args.monitor, terms=True)


def randomize_args(args):
    """the dict for build_environment(randomize=...) of the --randomize, --rand_scale, --rand_push, --command_range and
    --command_interval flags, None when --randomize is not given"""
    if args.randomize is None:
        return None
    return dict(preset=args.randomize, scale=args.rand_scale, push=args.rand_push, command_range=args.command_range,
                command_interval=args.command_interval)


def start_state_args(args):
    """the dict for build_environment(start_state=...) of the --start_noise, --start_scale and --start_clearance flags, None when
    --start_noise is not given"""
    if args.start_noise is None:
        return None
    return dict(preset=args.start_noise, scale=args.start_scale, clearance=args.start_clearance)


def distill_args(args):
    """the dict for train(distill=...) of the --distill, --teacher_rows, --distill_loss and --dagger_beta flags, None without --distill"""
    if args.distill is None:
        return None
    b = list(args.dagger_beta or []) + [1.0, 0.9][len(args.dagger_beta or []):]
    return dict(teacher=args.distill, rows=args.teacher_rows, loss=args.distill_loss, beta=b[0], decay=b[1])


def termination_args(args):
    """the dict for TrexVecEnv(terminate=...) of the --terminate_* flags, None when none is given"""
    contact = [l for l in (args.terminate_contact or "").split(",") if l]
    if args.terminate_head_height is None and args.terminate_tilt is None and not contact:
        return None
    return dict(head_height=args.terminate_head_height, max_tilt=args.terminate_tilt, keep_clear=contact or None,
                penalty=args.fall_penalty)


def environment_from_args(args):
    """the env the flags ask for (main's; the --terminate_* flags included)"""
    terminate = termination_args(args)
    env = build_environment(args.num_envs, max_episode_steps=args.max_episode_steps, warmstart=args.warmstart,
                            push_force=args.push_force, push_interval=args.push_interval, push_duration=args.push_duration,
                            seed=args.random_seed, control_mode=None if args.control_mode == "position" else args.control_mode,
                            gain_scale=args.gain_scale, observations=args.observations, rewards=args.rewards, command=args.command,
                            motion=None if args.motion is None else dict(clip=args.motion, rsi=args.rsi, weight=args.motion_weight,
                                                                              mirror_clip=args.mirror_clip),
                            sensing=sensing_args(args), randomize=randomize_args(args), monitor=monitor_args(args), critic=args.critic,
                            start_state=start_state_args(args))
    if terminate is not None:   # (set on the built env: 'auto' needs its model - every body that does not stand on the floor at the start)
        if terminate["keep_clear"] == ["auto"]:
            from .termination import fall_bodies
            terminate["keep_clear"] = fall_bodies(env)
        env.set_termination(**terminate)
    return env


def mpc_args(args):
    """the dict for run_mpc(...) of the --mpc flags, None without --mpc"""
    if args.mpc is None:
        return None
    pick = lambda v, default: default if v is None else v
    return dict(samples=args.mpc[0], horizon=args.mpc[1], knots=args.mpc_knots, sigma=pick(args.mpc_sigma, 0.1),
                temperature=pick(args.mpc_temperature, 0.1), iterations=pick(args.mpc_iterations, 1), steps=pick(args.mpc_steps, 100),
                save_clip=args.save_clip, frames=args.frames, graphs=args.graphs, seed=args.random_seed)


def run_mpc(env, samples, horizon, knots=None, sigma=0.1, temperature=0.1, iterations=1, steps=100, save_clip=None, frames=None,
            graphs=False, seed=0, log=print, env_index=0, frame_size=(960, 720)):
    """Control every env of `env` with trex_gym.planner.Planner for `steps` control steps -> (states [T, N, W], rewards [T, N]).
    save_clip: an .npz of the states and the frame time, for motion.Clip.from_states; frames: a directory for one PNG per step."""
    import numpy as np
    from .planner import Planner
    env.reset_tensor()
    planner = Planner(env, samples, horizon, knots=knots, sigma=sigma, temperature=temperature, iterations=iterations, seed=seed,
                      use_graphs=graphs)
    if frames is not None:
        Image = _png_writer()
        os.makedirs(frames, exist_ok=True)
    states, rewards = [], []
    for t in range(int(steps)):
        states.append(env.get_state())
        _, rew, _ = planner.step()
        rewards.append(rew.clone())
        if frames is not None:
            rgb = env.render_tensor([env_index], frame_size[0], frame_size[1], None)[0].cpu().numpy()
            Image.fromarray(rgb).save(os.path.join(frames, "%05d-of-%05d.png" % (t, int(steps))))
    states, rewards = torch.stack(states).cpu().numpy(), torch.stack(rewards).cpu().numpy()
    log("MPC: %d steps, %d samples x %d steps per plan, mean return %.3f" % (len(rewards), samples, horizon, float(rewards.sum(0).mean())))
    if save_clip:
        dt = env.model.get_param("dt") * env.model.get_param("substeps")
        np.savez_compressed(save_clip, states=states.astype(np.float32), frame_dt=np.float64(dt))
    planner.close()
    return states, rewards


def main(argv=None):
    args = parse_args(argv)
    env = environment_from_args(args)
    mpc = mpc_args(args)
    if mpc is not None:
        run_mpc(env, **mpc)
        return
    agent, _ = train(env, args.num_timesteps, args.random_seed, args.nsteps, args.noptepochs, args.save, use_graphs=args.graphs,
                     preset=args.preset, distill=distill_args(args), symmetry=args.symmetry,
                     sym_coef=args.sym_coef)
    if args.play:
        if env.critic_rows is not None:         # (playing runs the policy alone: the critic row is no longer filled)
            from . import critic as critics
            critics.attach(env, None)
        if args.no_sensing and env.sense_api is not None:    # (the env the policy was trained in, its sensors taken off)
            from . import sensing as S
            S.attach(env, None)
        if args.no_randomize and env.random_api is not None:  # (likewise its episode randomisation)
            from . import randomize as Z
            Z.attach(env, None)
        if args.no_start_noise and env.start_api is not None:  # (likewise its start-state randomisation)
            from . import start_state as SS
            SS.attach(env, None)
        play(agent, args.num_play_timesteps, args.export, symmetric=args.symmetric, deterministic=args.play_deterministic,
             update_stats=not args.play_deterministic,
             frames_dir=args.frames)


if __name__ == "__main__":
    sys.exit(main())
