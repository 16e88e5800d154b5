"""The episode monitor of a TrexVecEnv, attached by attach(env, window, terms) (include/trex_monitor.h): what baselines' bench.Monitor
keeps for ppo2's eprewmean / eplenmean - the return and the length of every finished episode, a window of the last `window` of them
- and, beyond it, why each episode ended and the per-term sums of the reward and motion terms, kept on the device by two launches
per step behind the step call, so that a captured rollout replays.

    attach(env, window=100, terms=True)     the env gets `monitor_api` and `monitor`; window None takes it off again
    episode_stats(env)                      the window's summary as a dict: ONE device-to-host copy
    last_episode(env)                       every env's last finished episode, tensors on the device

Deviations, stated once: the window is per process (a sharded run merges the ranks' windows in the trainer); returns are summed in
f64, as Monitor sums Python floats, and recorded as f32; an episode abandoned by reset_tensor(mask) is not counted."""
import math

from . import monitor_capi as M


def attach(env, window=100, terms=True):
    """Give the env an episode monitor (TrexVecEnv._set_monitor): every step_tensor applies it on the step's own rows behind the
    reward compose and the motion step, reset_tensor(mask) abandons the running episode of the envs it resets, step_many_tensor
    applies once per step block. terms: also sum the env's reward_terms and motion_terms blocks per episode (as they are when
    this is called: attach after the rewards and the motion clip). The env then has `monitor_api` (monitor_capi.BatchMonitor) and
    `monitor`, the recorded settings dict(window=, terms=). The env offset is the env's first global env index. window None or 0
    takes it all off again."""
    env._set_monitor(window, terms=terms)
    return env


def _api(env):
    api = getattr(env, "monitor_api", None)
    if api is None:
        raise ValueError("the env has no monitor (trex_gym.monitor.attach)")
    return api


def column_names(env):
    """the names of the monitor's columns: the reward terms', then the motion terms'"""
    api = _api(env)
    return list(env.reward_names)[:api.cols_a] + list(env.motion_names)[:api.cols_b]


def stats_from_summary(values, names=()):
    """the summary's numbers (a sequence of SUMMARY + C floats, monitor_capi's layout) as the dict episode_stats returns"""
    v = [float(x) for x in values]
    n = int(v[M.N])
    share = lambda k: v[M.WIN_REASON + k] / n if n else math.nan
    return {
        "eprewmean": v[M.RET_MEAN], "eplenmean": v[M.LEN_MEAN], "episodes": int(v[M.TOTAL]), "window_episodes": n,
        "epretmin": v[M.RET_MIN], "epretmax": v[M.RET_MAX], "eplenmin": v[M.LEN_MIN], "eplenmax": v[M.LEN_MAX],
        "end_reasons": {name: share(k) for k, name in enumerate(M.REASON_NAMES)},
        "end_counts": {name: int(v[M.BY_REASON + k]) for k, name in enumerate(M.REASON_NAMES)},
        "calls": int(v[M.T]),
        "terms": {name: v[M.SUMMARY + c] for c, name in enumerate(names)},
    }


def merge_summaries(parts):
    """the summaries of several ranks (sequences of SUMMARY + C floats) as one: the windows' sums and counts added - a mean over
    all ranks' windows, each weighted by its n -, extrema taken over all, totals and calls added up (calls: the largest). A rank
    whose window is empty contributes nothing."""
    parts = [[float(x) for x in p] for p in parts]
    out = [math.nan] * len(parts[0])
    live = [p for p in parts if p[M.N] > 0]
    n = sum(p[M.N] for p in live)
    out[M.N] = n
    means = [M.RET_MEAN, M.LEN_MEAN] + list(range(M.SUMMARY, len(out)))
    if live:
        for k in means:
            out[k] = sum(p[k] * p[M.N] for p in live) / n
        for k, pick in ((M.RET_MIN, min), (M.RET_MAX, max), (M.LEN_MIN, min), (M.LEN_MAX, max)):
            out[k] = pick(p[k] for p in live)
    for k in list(range(M.WIN_REASON, M.WIN_REASON + 4)) + [M.TOTAL] + list(range(M.BY_REASON, M.BY_REASON + 4)):
        out[k] = sum(p[k] for p in parts)
    out[M.T] = max(p[M.T] for p in parts)
    return out


def episode_stats(env):
    """-> dict: eprewmean, eplenmean (the means over the window's n = min(episodes, window) entries, NaN while n is 0), episodes
    (finished since attach), window_episodes (n), epretmin / epretmax / eplenmin / eplenmax, end_reasons {limit, head, tilt,
    clearance: share of the window; a fall with two criteria counts in both}, end_counts (the same as totals since attach), calls,
    and terms {name: mean per-episode sum of that reward or motion term}. One launch and one device-to-host copy."""
    api = _api(env)
    return stats_from_summary(api.summary().cpu().tolist(), column_names(env))


def last_episode(env):
    """-> dict of device tensors, one entry per env: `return` f32, `length`, `reason`, `t` (the apply call that finished it) int32,
    `cols` [n, C] f32 - zeros for an env that has finished none -, `episodes` int32 (finished so far), and the running episode's
    `running_return` f64 and `running_length` int32. Stream-ordered copies, nothing read back."""
    import torch
    api = _api(env)
    n, dev = env.num_envs, env.device
    i32 = lambda: torch.zeros(n, dtype=torch.int32, device=dev)
    out = {"return": torch.zeros(n, device=dev), "length": i32(), "reason": i32(), "t": i32(),
           "cols": torch.zeros(n, api.cols, device=dev), "episodes": i32(),
           "running_return": torch.zeros(n, dtype=torch.float64, device=dev), "running_length": i32()}
    api.info(last_return=out["return"], last_length=out["length"], last_reason=out["reason"], last_t=out["t"], last_cols=out["cols"],
             episodes=out["episodes"], ret=out["running_return"], len=out["running_length"])
    return out
