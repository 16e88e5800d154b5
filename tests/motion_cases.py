"""Procedural motion clips for the motion tests: sinusoids inside the joint limits, a base that translates and yaws. Seeded; numpy
only, no torch and no device, so that the host tests and the GPU tests take the same clips from here. A helper, not a conftest."""
import numpy as np

J = 25
DT = 1.0 / 32.0          # exact in f32, and so is every knot time k / 32


def yaw_quat(a):
    return np.array([0.0, 0.0, np.sin(0.5 * a), np.cos(0.5 * a)])


def quat_mul(a, b):
    x1, y1, z1, w1 = a
    x2, y2, z2, w2 = b
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def clip_frames(model, F, seed=0, frame_dt=DT, cyclic=False, amplitude=0.35, speed=0.8, yaw=1.2, tilt=0.1):
    """frames [F, 7 + J]: every joint a sinusoid of its own phase and whole number of periods over the clip, spanning `amplitude`
    of the half range around the middle of its limits; the base walks along x at `speed` with a sway in y and z, yaws by `yaw`
    rad over the clip and pitches by a `tilt` sinusoid. cyclic: frame F-1 repeats frame 0 but for the base's x and y (the yaw a
    sinusoid too), what a looping clip wants."""
    rng = np.random.default_rng(1000 + seed)
    oo = model["obs_order"]
    lo, hi = model["q_lower"][oo], model["q_upper"][oo]
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    nj = len(oo)
    s = np.arange(F) / (F - 1.0)                      # 0 .. 1 over the clip
    periods, phase = rng.integers(1, 4, nj), rng.uniform(0, 2 * np.pi, nj)
    q = mid + amplitude * half * np.sin(2 * np.pi * periods * s[:, None] + phase)
    T = (F - 1) * frame_dt
    frames = np.zeros((F, 7 + nj))
    frames[:, 0] = speed * T * s
    frames[:, 1] = 0.2 * np.sin(2 * np.pi * s) + 0.3 * T * s
    frames[:, 2] = 3.0 + 0.05 * np.sin(4 * np.pi * s)              # (the model's start height: the feet clear of the floor)
    heading = yaw * (np.sin(2 * np.pi * s) if cyclic else s)
    pitch = tilt * np.sin(2 * np.pi * s)
    for k in range(F):
        frames[k, 3:7] = quat_mul(yaw_quat(heading[k]), np.array([0.0, np.sin(0.5 * pitch[k]), 0.0, np.cos(0.5 * pitch[k])]))
    frames[:, 7:] = q
    return frames


def two_frame_clip(model, angle_deg, seed=0):
    """F = 2: the middle pose of the joints, then `amplitude` away; the base turns by angle_deg about a tilted axis between them"""
    f = clip_frames(model, 2, seed)
    axis = np.array([0.3, -0.2, 0.9])
    axis /= np.linalg.norm(axis)
    a = np.radians(angle_deg)
    f[1, 3:7] = quat_mul(np.concatenate([axis * np.sin(0.5 * a), [np.cos(0.5 * a)]]), f[0, 3:7])
    return f


def end_effector_links(model, K):
    """K (link index, xyz) pairs: toes first, then the head's link, then whatever moves, with points off the link origins"""
    names, lb = list(model["link_names"]), np.asarray(model["link_body"], int)
    toes = [l for l in range(len(names)) if "toe" in names[l]]
    head = [l for l in range(len(names)) if lb[l] == int(model["head_body"])][:1]
    rest = [l for l in range(len(names)) if lb[l] > 0 and l not in toes + head]
    links = (toes[:4] + head + rest)[:K]
    rng = np.random.default_rng(77)
    return [(int(l), tuple(rng.uniform(-0.2, 0.2, 3))) for l in links]
