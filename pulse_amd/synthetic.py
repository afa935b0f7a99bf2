"""Deterministic synthetic inputs for the PULSE hot path.

There is no AMASS data and no Isaac Gym here, so every rollout input is
synthetic: a "physics state" per step (the (N, 24, 13) rigid-body records Isaac
Gym would expose, phc/env/tasks/humanoid.py:215-222), the reference-motion frame
at time t (reward / reset) and t+1 (task observation), dof forces / velocities,
progress counters and episode-end flags.

Generation is on CPU with an explicit ``torch.Generator`` (seed 1234 + rank) so
that the CPU oracle and the HIP path consume bit-identical buffers; callers move
the result to the device.  This module is input plumbing, not part of the
measured path.
"""
import math

import torch

NUM_BODIES = 24          # SMPL_MUJOCO_NAMES, phc/env/tasks/humanoid.py:375-379
NUM_DOF = 69             # 23 joints x 3 exp-map dofs, humanoid.py:643-646
RB_WIDTH = 13            # pos 3, rot xyzw 4, lin vel 3, ang vel 3

SMPL_BODY_NAMES = ['Pelvis', 'L_Hip', 'L_Knee', 'L_Ankle', 'L_Toe', 'R_Hip', 'R_Knee', 'R_Ankle', 'R_Toe',
                   'Torso', 'Spine', 'Chest', 'Neck', 'Head', 'L_Thorax', 'L_Shoulder', 'L_Elbow', 'L_Wrist',
                   'L_Hand', 'R_Thorax', 'R_Shoulder', 'R_Elbow', 'R_Wrist', 'R_Hand']
# env_im.yaml:38 reset_bodies (every body except the ankles / toes)
RESET_BODY_NAMES = ['Pelvis', 'L_Hip', 'L_Knee', 'R_Hip', 'R_Knee', 'Torso', 'Spine', 'Chest', 'Neck', 'Head',
                    'L_Thorax', 'L_Shoulder', 'L_Elbow', 'L_Wrist', 'L_Hand', 'R_Thorax', 'R_Shoulder',
                    'R_Elbow', 'R_Wrist', 'R_Hand']
RESET_BODY_IDS = [SMPL_BODY_NAMES.index(n) for n in RESET_BODY_NAMES]
VR_TRACK_BODY_IDS = [SMPL_BODY_NAMES.index(n) for n in ('Head', 'L_Hand', 'R_Hand')]  # env_pulse_im.yaml:71-72


# SMPL-X / SMPL-H: 52 bodies, 153 dofs (humanoid.py:376-377, robot/smplx_humanoid.yaml).  The reference takes the list from smpl_sim
# (SMPLH_MUJOCO_NAMES); here the names are written in the order in which the reference itself spells them (humanoid.py:406-411,
# humanoid_im.py:628).  The order matters only for name-to-index lookups (track / reset / key bodies): the kernels see indices.
_FINGERS = [f"{f}{k}" for f in ("Index", "Middle", "Pinky", "Ring", "Thumb") for k in (1, 2, 3)]
SMPLX_BODY_NAMES = (['Pelvis', 'L_Hip', 'L_Knee', 'L_Ankle', 'L_Toe', 'R_Hip', 'R_Knee', 'R_Ankle', 'R_Toe',
                     'Torso', 'Spine', 'Chest', 'Neck', 'Head', 'L_Thorax', 'L_Shoulder', 'L_Elbow', 'L_Wrist'] + ["L_" + f for f in _FINGERS] +
                    ['R_Thorax', 'R_Shoulder', 'R_Elbow', 'R_Wrist'] + ["R_" + f for f in _FINGERS])


def _smplx_parents():
    """Legs, spine chain and arms as in the SMPL tree; every finger a chain of three rooted at the wrist."""
    par = [-1, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 12]
    for _ in ("L", "R"):
        base = len(par)                                   # the thorax
        par += [11, base, base + 1, base + 2]
        wrist = base + 3
        for f in range(5):
            first = wrist + 1 + 3 * f
            par += [wrist, first, first + 1]
    return par


def _skeleton(names, parents, dof_removed, reset_excluded):
    return {"body_names": list(names), "parents": list(parents), "num_bodies": len(names), "num_dof": 3 * (len(names) - 1),
            # dof_subset (humanoid.py:396-421): the dofs of every joint but the removed ones
            "dof_subset": [3 * (i - 1) + k for i, b in enumerate(names) if i > 0 and b not in dof_removed for k in range(3)],
            "track_bodies": list(names),                                                   # full-body tracking
            "reset_bodies": [b for b in names if b not in reset_excluded],                 # every body except the ankles / toes
            "key_bodies": ["R_Ankle", "L_Ankle", "R_Wrist", "L_Wrist"]}


def skeleton(humanoid="smpl"):
    """The description of a humanoid: a key of SKELETONS ('smpl' | 'smplh' | 'smplx') or a description dict itself."""
    if isinstance(humanoid, dict):
        return humanoid
    if humanoid not in SKELETONS:
        raise NotImplementedError(f"humanoid_type {humanoid!r}: 'smpl', 'smplh' and 'smplx' are built (humanoid.py:374-377)")
    return SKELETONS[humanoid]


def make_generator(seed=1234, rank=0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed + rank)
    return g


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float32)


def _quat_mul_xyzw(a, b):
    # plain 16-multiply Hamilton product; only used to CONSTRUCT inputs
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([
        aw * bx + ax * bw + ay * bz - az * by,
        aw * by - ax * bz + ay * bw + az * bx,
        aw * bz + ax * by - ay * bx + az * bw,
        aw * bw - ax * bx - ay * by - az * bz], dim=-1)


def rigid_body_state(g, n, j=NUM_BODIES):
    """(n, j, 13) records: root xy ~ N(0,1), root z ~ U(.75,1), others root + N(0,.3^2)."""
    rb = torch.empty(n, j, RB_WIDTH, dtype=torch.float32)
    root = torch.cat([_randn(g, n, 2), 0.75 + 0.25 * _rand(g, n, 1)], dim=-1)
    pos = root[:, None, :] + 0.3 * _randn(g, n, j, 3)
    pos[:, 0] = root
    rb[..., 0:3] = pos
    q = _randn(g, n, j, 4)
    rb[..., 3:7] = q / q.norm(dim=-1, keepdim=True)
    rb[..., 7:10] = _randn(g, n, j, 3)
    rb[..., 10:13] = 2.0 * _randn(g, n, j, 3)
    return rb


def reference_frame(g, rb, pos_sigma=0.05, max_angle=0.3, vel_sigma=0.1):
    """A reference-motion frame near ``rb``: dict pos/rot/vel/ang, each (n, j, .)."""
    n, j, _ = rb.shape
    ang = max_angle * _rand(g, n, j)
    ax = _randn(g, n, j, 3)
    ax = ax / ax.norm(dim=-1, keepdim=True)
    dq = torch.cat([ax * torch.sin(0.5 * ang)[..., None], torch.cos(0.5 * ang)[..., None]], dim=-1)
    rot = _quat_mul_xyzw(dq, rb[..., 3:7])
    rot = rot / rot.norm(dim=-1, keepdim=True)
    return {
        "pos": (rb[..., 0:3] + pos_sigma * _randn(g, n, j, 3)).contiguous(),
        "rot": rot.contiguous(),
        "vel": (rb[..., 7:10] + vel_sigma * _randn(g, n, j, 3)).contiguous(),
        "ang": (rb[..., 10:13] + vel_sigma * _randn(g, n, j, 3)).contiguous(),
    }


def env_step_inputs(g, n, edge_cases=True, humanoid="smpl"):
    """All inputs of one HumanoidIm.post_physics_step for n envs."""
    sk = skeleton(humanoid)
    rb = rigid_body_state(g, n, sk["num_bodies"])
    ref_now = reference_frame(g, rb)
    ref_next = reference_frame(g, rb)
    dof_force = 50.0 * _randn(g, n, sk["num_dof"])
    dof_vel = _randn(g, n, sk["num_dof"])
    progress = torch.randint(0, 300, (n,), generator=g, dtype=torch.int64)
    pass_time = _rand(g, n) < 0.02
    if edge_cases and n >= 8:
        # identical cur / ref rotation: w rounds to >= 1 -> NaN-mask branch of quat_to_angle_axis
        ref_now["rot"][0] = rb[0, :, 3:7]
        ref_next["rot"][0] = rb[0, :, 3:7]
        # antipodal quaternions (q vs -q)
        ref_now["rot"][1] = -rb[1, :, 3:7]
        ref_next["rot"][1] = -rb[1, :, 3:7]
        # progress <= 1 (no termination) and <= 3 (no power reward)
        progress[2] = 0
        progress[3] = 1
        progress[4] = 3
        progress[5] = 4
        # guaranteed far-away body -> termination when progress > 1
        ref_now["pos"][5, 13] += 1.0
        ref_now["pos"][3, 9] += 1.0      # far, but progress <= 1 -> not terminated
        # identity root rotation (heading 0) and a pure-yaw root
        rb[6, 0, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1.0])
        rb[7, 0, 3:7] = torch.tensor([0.0, 0.0, math.sin(0.6), math.cos(0.6)])
        pass_time[2] = True
    return {"rb": rb, "ref_now": ref_now, "ref_next": ref_next, "dof_force": dof_force,
            "dof_vel": dof_vel, "progress": progress, "pass_time": pass_time}


def rollout_scalars(g, t, n, done_p=0.02):
    """Stand-alone GAE inputs: rewards / values / next_values (t,n,1), dones (t,n) u8."""
    rewards = _rand(g, t, n, 1)
    values = _randn(g, t, n, 1)
    next_values = _randn(g, t, n, 1)
    dones = (_rand(g, t, n) < done_p)
    term = dones & (_rand(g, t, n) < 0.5)
    next_values = next_values * (1.0 - term.float()[..., None])
    return rewards, values, next_values, dones.to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# Synthetic motion library: the flat per-frame tables MotionLibBase builds from AMASS clips
# (phc/utils/motion_lib_base.py:287-316): gts/grs/lrs/gvs/gavs (F, 24, 3|4), dvs (F, 23, 3) plus per-motion
# length / fps / dt / frame count.  Clips are smooth random articulated motions of an SMPL-shaped kinematic tree
# (forward kinematics over SMPL_PARENTS), velocities by finite differences like SkeletonMotion does.
# ---------------------------------------------------------------------------------------------------------------------
SMPL_PARENTS = [-1, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 12, 11, 14, 15, 16, 17, 11, 19, 20, 21, 22]
SMPLX_PARENTS = _smplx_parents()

_ANKLES_TOES = ("L_Ankle", "L_Toe", "R_Ankle", "R_Toe")
SKELETONS = {"smpl": _skeleton(SMPL_BODY_NAMES, SMPL_PARENTS, ("L_Hand", "R_Hand", "L_Toe", "R_Toe"), _ANKLES_TOES),
             "smplx": _skeleton(SMPLX_BODY_NAMES, SMPLX_PARENTS, ("L_Toe", "R_Toe"), _ANKLES_TOES)}       # humanoid.py:404-405
SKELETONS["smplh"] = SKELETONS["smplx"]                                                                  # humanoid.py:376: the same 52 bodies

# SMPL's own joint order under the humanoid's body names: the order of a raw SMPL pose row (F, 72).  The reference takes the list from
# smpl_sim (SMPL_BONE_ORDER_NAMES, convert_amass_data.py:16, 104); it is the public SMPL kinematic tree.
SMPL_BONE_ORDER_NAMES = ['Pelvis', 'L_Hip', 'R_Hip', 'Torso', 'L_Knee', 'R_Knee', 'Spine', 'L_Ankle', 'R_Ankle', 'Chest', 'L_Toe', 'R_Toe',
                         'Neck', 'L_Thorax', 'R_Thorax', 'Head', 'L_Shoulder', 'R_Shoulder', 'L_Elbow', 'R_Elbow', 'L_Wrist', 'R_Wrist',
                         'L_Hand', 'R_Hand']


def smpl_joint_map(body_names=None):
    """smpl_2_mujoco (convert_amass_data.py:104): for every body of the humanoid, in body order, the SMPL joint it takes its rotation from."""
    names = SMPL_BODY_NAMES if body_names is None else body_names
    return [SMPL_BONE_ORDER_NAMES.index(q) for q in names if q in SMPL_BONE_ORDER_NAMES]


def mirror_body_map(body_names=None):
    """left_to_right_index (convert_amass_isaac.py:121): every L_ body takes its R_ twin's place and the other way round."""
    names = list(SMPL_BODY_NAMES if body_names is None else body_names)
    swap = {"L_": "R_", "R_": "L_"}
    return [names.index(swap[n[:2]] + n[2:]) if n[:2] in swap else i for i, n in enumerate(names)]


def _exp_map_to_quat_xyzw(e):
    ang = e.norm(dim=-1, keepdim=True)
    half = 0.5 * ang
    k = torch.where(ang > 1e-8, torch.sin(half) / ang.clamp_min(1e-8), torch.full_like(ang, 0.5))
    return torch.cat([e * k, torch.cos(half)], dim=-1)


def _quat_rotate_xyzw(q, v):
    qv, w = q[..., :3], q[..., 3:4]
    t = 2.0 * torch.cross(qv, v, dim=-1)
    return v + w * t + torch.cross(qv, t, dim=-1)


def motion_shape_rows(g, num_motions):
    """Per-motion body-shape rows as the reference's motion library carries them (motion_lib_base.py:289, 294: _motion_bodies (M, 17) = [gender, 10 betas,
    6 unused], _motion_limb_weights (M, 10)); every column non-constant.  Draws from ``g`` only."""
    bodies = torch.cat([torch.randint(0, 2, (num_motions, 1), generator=g).float(), _randn(g, num_motions, 10), _rand(g, num_motions, 6)], dim=-1)
    limb = _rand(g, num_motions, 10) + 0.5
    return bodies.contiguous(), limb.contiguous()


def synthetic_motion_library(g, num_motions, min_frames=45, max_frames=180, fps=30.0, humanoid="smpl", shape_rows=False, shape_seed=7117):
    """dict of CPU tensors in the reference's table layout; frame f of motion m sits at length_starts[m] + f.  ``humanoid``: a key of
    SKELETONS or a description dict (``parents`` is all that is read: any tree whose parents precede their children).
    ``shape_rows``: also ``motion_bodies`` (M, 17) / ``motion_limb_weights`` (M, 10), drawn from a generator of their own (``shape_seed``) so
    that the tables are the same draw for draw with and without them."""
    sk = skeleton(humanoid)
    parents = sk["parents"]
    m, j = num_motions, len(parents)
    num_frames = torch.randint(min_frames, max_frames + 1, (m,), generator=g, dtype=torch.int64)
    starts = torch.cumsum(num_frames, 0) - num_frames
    total = int(num_frames.sum())
    mid = torch.repeat_interleave(torch.arange(m), num_frames)                     # motion of every frame
    fidx = torch.arange(total) - starts[mid]
    dt = 1.0 / fps
    t = (fidx.float() * dt)[:, None, None]                                         # (F,1,1)
    # joint exp-map trajectories: two sinusoids per dof
    amp = 0.35 * _rand(g, m, j, 3, 2)
    amp[:, 0] *= 0.3                                                               # pelvis tilt stays small
    frq = 0.3 + 1.7 * _rand(g, m, j, 3, 2)
    pha = 6.2831853 * _rand(g, m, j, 3, 2)
    e = (amp[mid] * torch.sin(6.2831853 * frq[mid] * t[..., None] + pha[mid])).sum(-1)      # (F,24,3)
    yaw_rate = 0.8 * _randn(g, m)
    e[:, 0, 2] += 6.2831853 * _rand(g, m)[mid] + yaw_rate[mid] * t[:, 0, 0]
    lrs = _exp_map_to_quat_xyzw(e)
    lrs = lrs / lrs.norm(dim=-1, keepdim=True)
    offsets = 0.08 + 0.3 * _rand(g, j, 3) * torch.tensor([0.4, 0.4, 1.0])
    offsets[0] = 0.0
    # root path: constant drift + sway
    drift = 0.6 * _randn(g, m, 3) * torch.tensor([1.0, 1.0, 0.0])
    sway = 0.05 * _randn(g, m, 3)
    root = drift[mid] * t[:, 0] + sway[mid] * torch.sin(3.0 * t[:, 0]) + torch.tensor([0.0, 0.0, 0.9])
    grs = torch.empty(total, j, 4)
    gts = torch.empty(total, j, 3)
    for b in range(j):
        p = parents[b]
        if p < 0:
            grs[:, b], gts[:, b] = lrs[:, b], root
        else:
            grs[:, b] = _quat_mul_xyzw(grs[:, p], lrs[:, b])
            gts[:, b] = gts[:, p] + _quat_rotate_xyzw(grs[:, p], offsets[b].expand(total, 3))
    grs = grs / grs.norm(dim=-1, keepdim=True)

    def fdiff(x):                                                                  # forward difference inside each clip, last frame repeats
        nxt = torch.roll(x, -1, 0)
        d = (nxt - x) / dt
        last = fidx == (num_frames[mid] - 1)
        d[last] = d[torch.where(last)[0] - 1]
        return d

    def ang_vel(q):                                                                # 2 (q_{f+1} conj(q_f)).xyz / dt
        nxt = torch.roll(q, -1, 0)
        conj = q * torch.tensor([-1.0, -1.0, -1.0, 1.0])
        dq = _quat_mul_xyzw(nxt, conj)
        dq = torch.where(dq[..., 3:4] < 0, -dq, dq)
        w = 2.0 * dq[..., :3] / dt
        last = fidx == (num_frames[mid] - 1)
        w[last] = w[torch.where(last)[0] - 1]
        return w

    gvs, gavs = fdiff(gts), ang_vel(grs)
    dvs = ang_vel(lrs)[:, 1:]
    tables = {
        "gts": gts.contiguous(), "grs": grs.contiguous(), "lrs": lrs.contiguous(), "gvs": gvs.contiguous(),
        "gavs": gavs.contiguous(), "dvs": dvs.contiguous(),
        "motion_num_frames": num_frames, "motion_fps": torch.full((m,), fps), "motion_dt": torch.full((m,), dt),
        "motion_lengths": ((1.0 / fps) * (num_frames - 1).double()).float(), "length_starts": starts,   # curr_len, motion_lib_base.py:263
    }
    if shape_rows:
        tables["motion_bodies"], tables["motion_limb_weights"] = motion_shape_rows(make_generator(shape_seed), m)
    return tables


def synthetic_motion_data(g, num_clips, humanoid="smpl", frames=None, min_frames=45, max_frames=180, fps=30, num_slots=None):
    """Raw motion data as the reference's motion file holds it (MotionLibBase.load_data, motion_lib_base.py:129-156), and skeleton trees to load it
    with: ``(data, (parents, local_translation (num_slots, J, 3)))``.  ``data``: key -> {pose_quat_global (F, J, 4) float32 numpy, root_trans_offset
    (F, 3) float32 tensor, pose_aa (F, J * 3), fps, [beta (10)]}: smooth random articulated clips (the joint trajectories of
    ``synthetic_motion_library``), every second clip marked with ``beta``.  ``frames``: the clips' lengths (default: drawn in
    [min_frames, max_frames]); ``fps``: one value or one per clip.  ``num_slots`` skeletons (default num_clips) share the parents and differ in
    their bone offsets, as bodies of different shape do.  For ``MotionLib.from_motion_data``."""
    sk = skeleton(humanoid)
    parents = sk["parents"]
    m, j = num_clips, len(parents)
    num_frames = torch.randint(min_frames, max_frames + 1, (m,), generator=g, dtype=torch.int64) if frames is None else torch.as_tensor(frames, dtype=torch.int64)
    fps_list = [fps] * m if not isinstance(fps, (list, tuple)) else list(fps)
    if num_frames.numel() != m or len(fps_list) != m:
        raise ValueError(f"synthetic_motion_data: {m} clips need {m} lengths and fps values")
    data = {}
    for c in range(m):
        f = int(num_frames[c])
        t = (torch.arange(f, dtype=torch.float32) / float(fps_list[c]))[:, None, None]
        amp = 0.35 * _rand(g, j, 3, 2)
        amp[0] *= 0.3
        frq = 0.3 + 1.7 * _rand(g, j, 3, 2)
        pha = 6.2831853 * _rand(g, j, 3, 2)
        e = (amp * torch.sin(6.2831853 * frq * t[..., None] + pha)).sum(-1)                     # (F, J, 3) joint exp maps
        e[:, 0, 2] += 6.2831853 * _rand(g, 1) + 0.8 * _randn(g, 1) * t[:, 0, 0]
        lrs = _exp_map_to_quat_xyzw(e)
        lrs = lrs / lrs.norm(dim=-1, keepdim=True)
        grs = torch.empty(f, j, 4)
        for b in range(j):
            grs[:, b] = lrs[:, b] if parents[b] < 0 else _quat_mul_xyzw(grs[:, parents[b]], lrs[:, b])
        grs = grs / grs.norm(dim=-1, keepdim=True)
        root = (0.6 * _randn(g, 3) * torch.tensor([1.0, 1.0, 0.0])) * t[:, 0] + 0.05 * _randn(g, 3) * torch.sin(3.0 * t[:, 0]) + torch.tensor([0.0, 0.0, 0.9])
        clip = {"pose_quat_global": grs.contiguous().numpy(), "root_trans_offset": root.contiguous(), "pose_aa": e.reshape(f, j * 3).contiguous().numpy(),
                "fps": fps_list[c]}
        if c % 2 == 0:
            clip["beta"] = _randn(g, 10).numpy()
        data[f"clip_{c:04d}"] = clip
    slots = m if num_slots is None else num_slots
    offsets = 0.08 + 0.3 * _rand(g, j, 3) * torch.tensor([0.4, 0.4, 1.0])
    lt = offsets[None] * (1.0 + 0.1 * _randn(g, slots, 1, 1))
    lt[:, 0] = 0.0
    return data, (list(parents), lt.contiguous())


def synthetic_smpl_data(g, num_clips, frames=None, min_frames=45, max_frames=180, framerate=30, num_slots=None):
    """Raw SMPL motion as data sets ship it, and skeleton trees to load it with: ``(data, (parents, local_translation (num_slots, 24, 3)))``.
    ``data``: key -> {poses (F, 72) float32 numpy axis-angle in SMPL joint order (hands included), trans (F, 3) float32 numpy, betas (16),
    gender, mocap_framerate}: two sinusoids per joint axis, a drifting and swaying root.  ``frames``: the RAW lengths (default: drawn in
    [min_frames, max_frames] x int(framerate / 30)); ``framerate``: one value or one per clip.  For ``MotionLib.from_smpl_data``."""
    import numpy as np
    m = num_clips
    rates = [framerate] * m if not isinstance(framerate, (list, tuple)) else list(framerate)
    if frames is None:
        frames = (torch.randint(min_frames, max_frames + 1, (m,), generator=g, dtype=torch.int64) * torch.tensor([max(1, int(r / 30)) for r in rates])).tolist()
    if len(frames) != m or len(rates) != m:
        raise ValueError(f"synthetic_smpl_data: {m} clips need {m} lengths and framerates")
    data = {}
    for c in range(m):
        f = int(frames[c])
        t = (torch.arange(f, dtype=torch.float32) / float(rates[c]))[:, None, None]
        amp = 0.35 * _rand(g, 24, 3, 2)
        amp[0] *= 0.3
        frq = 0.3 + 1.7 * _rand(g, 24, 3, 2)
        pha = 6.2831853 * _rand(g, 24, 3, 2)
        e = (amp * torch.sin(6.2831853 * frq * t[..., None] + pha)).sum(-1)                     # (F, 24, 3) joint axis-angles
        e[:, 0, 2] += 6.2831853 * _rand(g, 1) + 0.8 * _randn(g, 1) * t[:, 0, 0]
        root = (0.6 * _randn(g, 3) * torch.tensor([1.0, 1.0, 0.0])) * t[:, 0] + 0.05 * _randn(g, 3) * torch.sin(3.0 * t[:, 0]) + torch.tensor([0.0, 0.0, 0.9])
        data[f"clip_{c:04d}"] = {"poses": e.reshape(f, 72).contiguous().numpy(), "trans": root.contiguous().numpy(), "betas": _randn(g, 16).numpy(),
                                 "gender": np.array("neutral"), "mocap_framerate": np.array(float(rates[c]))}
    slots = m if num_slots is None else num_slots
    offsets = 0.08 + 0.3 * _rand(g, 24, 3) * torch.tensor([0.4, 0.4, 1.0])
    lt = offsets[None] * (1.0 + 0.1 * _randn(g, slots, 1, 1))
    lt[:, 0] = 0.0
    return data, (list(SMPL_PARENTS), lt.contiguous())


def synthetic_mdm_result(g, num_clips, frames=196, num_slots=None, jitter=0.0, spin=9.0):
    """What a text-to-motion model hands back (the ``res_data["json_file"]`` layout scripts/data_process/convert_data_mdm.py:48-51 reads), and
    skeleton trees to load it with: ``(result, (parents, local_translation (num_slots, 24, 3)))``.  ``result``: {thetas: ``num_clips`` arrays
    (F, 24, 3) float32, per-joint Euler 'XYZ' angles in DEGREES in SMPL joint order; root_translation: ``num_clips`` arrays (F, 3) float32, y up}.
    ``frames``: one length or one per clip (196 is what MDM emits).  Every clip turns the root about the vertical by about ``spin`` degrees
    a frame, and swings one shoulder around a half turn: the rotation angle of the root and of that limb passes pi between consecutive
    frames, where the rotation-vector representation wraps and the converted quaternions change sign.  ``jitter``: standard deviation in
    degrees of white noise added to every angle (generated motion is jittery).  For ``MotionLib.from_mdm_data``."""
    m = num_clips
    lengths = [int(frames)] * m if not isinstance(frames, (list, tuple)) else [int(f) for f in frames]
    if len(lengths) != m:
        raise ValueError(f"synthetic_mdm_result: {m} clips need {m} lengths")
    shoulder = SMPL_BONE_ORDER_NAMES.index("L_Shoulder")
    thetas, roots = [], []
    for c in range(m):
        f = lengths[c]
        t = torch.arange(f, dtype=torch.float32)[:, None, None] / 30.0
        amp = 18.0 * _rand(g, 24, 3, 2)
        frq = 0.3 + 1.7 * _rand(g, 24, 3, 2)
        pha = 6.2831853 * _rand(g, 24, 3, 2)
        e = (amp * torch.sin(6.2831853 * frq * t[..., None] + pha)).sum(-1)                     # (F, 24, 3) degrees
        e[:, 0, 1] += 360.0 * _rand(g, 1) + (spin * (1.0 + 0.3 * _rand(g, 1))) * 30.0 * t[:, 0, 0]        # y is up before the script's +90 degrees about x
        e[:, shoulder, 0] += 180.0 + 35.0 * torch.sin(6.2831853 * (1.5 + _rand(g, 1)) * t[:, 0, 0] + 6.2831853 * _rand(g, 1))
        if jitter:
            e = e + float(jitter) * _randn(g, f, 24, 3)
        tt = t[:, 0]
        root = (0.6 * _randn(g, 3) * torch.tensor([1.0, 0.0, 1.0])) * tt + 0.05 * _randn(g, 3) * torch.sin(3.0 * tt) + torch.tensor([0.0, 0.9, 0.0])
        if jitter:
            root = root + 0.002 * float(jitter) * _randn(g, f, 3)
        thetas.append(e.contiguous().numpy())
        roots.append(root.contiguous().numpy())
    slots = m if num_slots is None else num_slots
    offsets = 0.08 + 0.3 * _rand(g, 24, 3) * torch.tensor([0.4, 0.4, 1.0])
    lt = offsets[None] * (1.0 + 0.1 * _randn(g, slots, 1, 1))
    lt[:, 0] = 0.0
    return {"thetas": thetas, "root_translation": roots}, (list(SMPL_PARENTS), lt.contiguous())


# --------------------------------------------------------------------------- #
# Action-dependent physics stand-in (return-parity experiments): constants shared by the HIP kernel's host class
# (pulse_amd/env/sim.py:PdSim) and its CPU twin (oracle/pd_sim_oracle.py).  See include/pulse_hip.h: pulse_pd_sim_args.
# --------------------------------------------------------------------------- #
PD_SIM = {"kp": 400.0, "kd": 40.0, "substeps": 2, "action_scale": 0.25, "lever": 0.3, "noise_acc": 2.0}


def synthetic_dof_limits(humanoid="smpl", seed=0):
    """Joint limits a simulator would publish (Isaac's get_actor_dof_properties, humanoid.py:867-896): (lower, upper), two (D,) float32 CPU
    tensors with lower < upper.  Half-widths in 0.3 .. 3.0 rad, so that some joints' 1.2 max|limit| passes pi and others' does not (the cap of
    _build_pd_action_offset_scale, humanoid.py:1050-1054); about half of the dofs are off-centre, so the two bias_offset branches differ."""
    sk = skeleton(humanoid)
    g = make_generator(9100 + seed)
    d = sk["num_dof"]
    half = 0.3 + 2.7 * _rand(g, d)
    centre = torch.where(_rand(g, d) < 0.5, (_rand(g, d) - 0.5) * half, torch.zeros(d))
    return (centre - half).contiguous(), (centre + half).contiguous()


def pd_sim_tables(humanoid="smpl"):
    """(sag (num_dof,), lever_dir (num_bodies, 3)): a constant per-joint offset of the PD set point the policy has to learn to cancel, and the
    unit 'bone' directions that turn a joint-angle error into a body displacement.  Deterministic (no RNG state involved)."""
    sk = skeleton(humanoid)
    j = torch.arange(sk["num_dof"], dtype=torch.float32)
    sag = 0.25 * torch.sin(0.7 * (j + 1.0))
    b = torch.arange(sk["num_bodies"], dtype=torch.float32)
    u = torch.stack([torch.cos(1.3 * b), torch.sin(1.3 * b) * torch.cos(0.9 * b + 0.4), torch.sin(1.3 * b) * torch.sin(0.9 * b + 0.4)], dim=-1)
    return sag, u / u.norm(dim=-1, keepdim=True)


def synthetic_height_field(rows=260, cols=300, seed=5):
    """A height field with slopes, steps and noise in Isaac Gym's storage format (int16 samples, vertical scale 0.005 m, cells of 0.1 m):
    the stand-in for Terrain.heightsamples (phc/env/tasks/humanoid_pedestrian_terrain.py:1114-1160 builds it with isaacgym.terrain_utils,
    a closed third-party package)."""
    g = torch.Generator().manual_seed(seed)
    x, y = torch.meshgrid(torch.arange(rows).float(), torch.arange(cols).float(), indexing="ij")
    h = 0.6 * torch.sin(x / 23.0) * torch.cos(y / 31.0) + 0.15 * torch.floor(x / 40.0) + 0.05 * torch.randn(rows, cols, generator=g)
    return torch.round(h / 0.005).to(torch.int16)


def synthetic_poles(sub, difficulty, generator):
    """A deterministic stand-in for isaacgym.terrain_utils.poles_terrain (a closed third-party package; the reference calls it at
    phc/env/tasks/humanoid_pedestrian_terrain.py:1363, 1444) so that a terrain with obstacles can be built from nothing but a seed:
    2 + 10 * difficulty discs of radius 0.2 .. 0.5 m and height 1 .. 2.5 m on the flat sub-terrain ``sub`` (``height_field_raw`` (width,
    length) int16, written in place), none within 1.5 m of its centre, where the env origin is.  Draws come from ``generator``."""
    import numpy as np
    w, l = sub.height_field_raw.shape
    hs, vs = float(sub.horizontal_scale), float(sub.vertical_scale)
    num = 2 + int(10 * float(difficulty))
    u = _rand(generator, num, 4).double().numpy()
    rows, cols = np.meshgrid(np.arange(w), np.arange(l), indexing="ij")
    for ux, uy, ur, uh in u:
        cx, cy = ux * (w - 1), uy * (l - 1)
        if np.hypot(cx - (w - 1) / 2, cy - (l - 1) / 2) * hs < 1.5:
            continue
        disc = np.hypot(rows - cx, cols - cy) * hs <= 0.2 + 0.3 * ur
        sub.height_field_raw[disc] = np.int16(round((1.0 + 1.5 * uh) / vs))
    return sub


def square_height_points(extent=2.0, res=32):
    """init_square_height_points (humanoid_pedestrian_terrain.py:608-625): res x res grid over [-extent, extent]^2, x-major -> (res^2, 2)."""
    import numpy as np
    x = torch.tensor(np.linspace(-extent, extent, res))
    gx, gy = torch.meshgrid(x, x.clone(), indexing="ij")
    return torch.stack([gx.flatten(), gy.flatten()], dim=1).float()


def center_height_points():
    """init_center_height_points (:591-606): x in linspace(-0.1, 0.1, 3), y in linspace(-0.2, 0.2, 3) -> (9, 2)."""
    import numpy as np
    x, y = torch.tensor(np.linspace(-0.1, 0.1, 3)), torch.tensor(np.linspace(-0.2, 0.2, 3))
    gx, gy = torch.meshgrid(x, y, indexing="ij")
    return torch.stack([gx.flatten(), gy.flatten()], dim=1).float()


def synthetic_pnn_checkpoint(num_prim=4, in_dim=934, units=(96, 64), num_actions=69, seed=0, has_lateral=False):
    """A seeded stand-in for a trained PNN checkpoint (output/phc_kp_pnn_iccv/Humanoid.pth) with the keys ``load_pnn`` reads
    (phc/learning/network_loader.py:54-73): ``a2c_network.pnn.actors.<k>.<2i>.{weight,bias}``, with ``has_lateral`` the bias-free lateral
    links ``a2c_network.pnn.u.<i>.<j>.{0,1}.weight`` (pnn.py:24-37), ``a2c_network.mu.bias`` (the action size) and ``running_mean_std``."""
    g = make_generator(seed)
    units = list(units)
    pm = {}
    for k in range(num_prim):
        i = in_dim
        for li, u in enumerate(units + [num_actions]):
            pm[f"a2c_network.pnn.actors.{k}.{2 * li}.weight"] = _randn(g, u, i) / i ** 0.5
            pm[f"a2c_network.pnn.actors.{k}.{2 * li}.bias"] = 0.1 * _randn(g, u)
            i = u
    if has_lateral:
        if len(units) != 2:
            raise ValueError("lateral PNN columns have exactly two hidden layers (pnn.py:96)")
        for i in range(num_prim - 1):
            for j in range(i + 1):
                pm[f"a2c_network.pnn.u.{i}.{j}.0.weight"] = _randn(g, units[1], units[0]) / units[0] ** 0.5
                pm[f"a2c_network.pnn.u.{i}.{j}.1.weight"] = _randn(g, num_actions, units[-1]) / units[-1] ** 0.5
    pm["a2c_network.mu.weight"], pm["a2c_network.mu.bias"] = _randn(g, num_actions, units[-1]), _randn(g, num_actions)
    rms = {"running_mean": (0.3 * _randn(g, in_dim)).double(), "running_var": (_rand(g, in_dim) + 0.5).double(), "count": torch.tensor(1e4).double()}
    return {"model": pm, "running_mean_std": rms}
