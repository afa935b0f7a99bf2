"""A numpy restatement of what pulse_motion_export computes (include/pulse_hip.h section 2b'.2): the conversion lines of HumanoidIm.render
(phc/env/tasks/humanoid_im.py:217-257), the body of Humanoid._write_states_to_file (phc/env/tasks/humanoid.py:439-491) and the functions of
phc/utils/torch_utils.py they call, written out -- scipy's from_quat / __mul__ / as_rotvec, poselib's SkeletonState.local_rotation -- in fp64 by
default, with the un-normalised local products handed back beside the outputs, so that a test can look at the quaternions whose SIGN the
reference decides (quat_pos, w < 0).

    segments(progress (T, N))                        -> [(env, t0, frames)] in the reference's order (env-major, then time)
    export_frames(rb (F, J, 13), dof (F, 3 (J - 1)))  -> dict of per-frame fields
"""
import numpy as np

import motion_ingest_model as MI

UPRIGHT = (0.5, 0.5, 0.5, 0.5)
# recordings (T, N) beside the fixture's: one step, one env, a reset by exactly 1, resets at consecutive steps, a reset at the last step
EDGE_RECORDINGS = [[[7]], [[0], [1], [2], [0], [1]], [[3, 0], [4, 1], [5, 0], [0, 1]], [[5, 5, 5], [0, 6, 5], [0, 0, 5], [9, 1, 5]],
                   [[1, 2, 3, 4, 5, 6, 7, 8, 9, 0]]]
SENTINEL = -10


def segments(progress):
    """humanoid.py:444-470: the sentinel appended, a segment ends after step t where |progress[t] - progress[t + 1]| > 1."""
    progress = np.asarray(progress, dtype=np.int64)
    steps, envs = progress.shape
    out = []
    for e in range(envs):
        p = np.concatenate([progress[:, e], [SENTINEL]])
        ends = np.nonzero(np.abs(p[:-1] - p[1:]) > 1)[0] + 1
        start = 0
        for end in ends:
            out.append((e, int(start), int(end - start)))
            start = end
    return out


def segment_keys(segs):
    keys, count = [], {}
    for e, _, _ in segs:
        keys.append(f"{e}_{count.get(e, 0)}")
        count[e] = count.get(e, 0) + 1
    return keys


def normalize_angle(x):
    return np.arctan2(np.sin(x), np.cos(x))


def as_rotvec(q):
    """scipy Rotation.from_quat(q).as_rotvec(): normalise, w made >= 0, angle = 2 atan2(|xyz|, w), the series at angle <= 1e-3."""
    t = q.dtype.type
    q = MI.scipy_unit(q)
    q = np.where(q[..., 3:] < 0, -q, q)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    angle = t(2) * np.arctan2(np.sqrt(x * x + y * y + z * z), w)
    a2 = angle * angle
    small = t(2) + a2 / t(12) + t(7) * a2 * a2 / t(2880)
    with np.errstate(invalid="ignore", divide="ignore"):
        large = angle / np.sin(angle / t(2))
    scale = np.where(angle.astype(np.float64) <= 1e-3, small, large)
    return scale[..., None] * q[..., :3]


def quat_to_exp_map(q):
    """torch_utils.py:57-97: angle = normalize_angle(2 acos w), axis = xyz / sqrt(1 - w^2), (0, 0, 1) and angle 0 where that root is <= 1e-5."""
    t = q.dtype.type
    w = q[..., 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        st = np.sqrt(t(1) - w * w)
        angle = normalize_angle(t(2) * np.arccos(w))
        axis = q[..., :3] / st[..., None]
    ok = np.abs(st) > t(1e-5)
    default = np.zeros_like(axis)
    default[..., 2] = 1
    return np.where(ok, angle, t(0))[..., None] * np.where(ok[..., None], axis, default)


def exp_map_to_quat(e):
    """torch_utils.py:148-172 + isaacgym quat_from_angle_axis: normalised axis * sin(angle / 2), cos(angle / 2), the whole normalised."""
    t = e.dtype.type
    n = np.sqrt((e * e).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        axis = e / n[..., None]
    angle = normalize_angle(n)
    ok = np.abs(angle) > t(1e-5)
    default = np.zeros_like(axis)
    default[..., 2] = 1
    angle, axis = np.where(ok, angle, t(0)), np.where(ok[..., None], axis, default)
    axis = axis / np.maximum(np.sqrt((axis * axis).sum(-1, keepdims=True)), t(1e-9))
    h = angle / t(2)
    q = np.concatenate([axis * np.sin(h)[..., None], np.cos(h)[..., None]], axis=-1)
    return q / np.maximum(np.sqrt((q * q).sum(-1, keepdims=True)), t(1e-9))


def export_frames(rb, dof_pos, parents, joint_map, *, upright_start=True, root_offset=(0.0, 0.0, 0.0), dtype=np.float64):
    """Every frame of ``rb`` (F, J, 13) [and ``dof_pos`` (F, 3 (J - 1))] -> pose_quat_global, root_trans_offset (copies), upright (the globals
    in the SMPL frame), local_products, pose_quat, pose_aa (F, 3 J) in SMPL joint order, trans_orig, body_quat, dof_pos."""
    rb = np.asarray(rb, dtype=dtype)
    f, j = rb.shape[0], rb.shape[1]
    glob, root = rb[:, :, 3:7], rb[:, 0, 0:3]
    body_of_joint = [list(joint_map).index(s) for s in range(j)]
    out = {"pose_quat_global": glob.copy(), "root_trans_offset": root.copy(), "trans_orig": root - np.asarray(root_offset, dtype=dtype)}
    dof = None if dof_pos is None else np.asarray(dof_pos, dtype=dtype)
    if dof is not None:
        out["dof_pos"] = dof.copy()
        out["body_quat"] = np.concatenate([glob[:, :1], exp_map_to_quat(dof.reshape(f, j - 1, 3))], axis=1)
    if upright_start:
        up = MI.scipy_unit(MI.scipy_compose(MI.scipy_unit(glob), np.asarray(UPRIGHT, dtype=dtype)))
        lprod, pq = up.copy(), up.copy()
        conj = up * np.array([-1, -1, -1, 1], dtype=dtype)
        for b in range(1, j):
            lprod[:, b] = MI.quat_mul(conj[:, parents[b]], up[:, b])
            pq[:, b] = MI.quat_normalize(lprod[:, b])
        pq = pq.astype(np.float32).astype(dtype)        # poselib collects local_rotation in a float32 buffer whatever the state's dtype (skeleton3d.py:449)
        aa = as_rotvec(pq)
        out.update({"upright": up, "local_products": lprod})
    elif dof is not None:
        pq = out["body_quat"]
        aa = np.concatenate([quat_to_exp_map(glob[:, 0])[:, None], dof.reshape(f, j - 1, 3)], axis=1)
    else:
        return out
    out.update({"pose_quat": pq, "pose_aa": aa[:, body_of_joint].reshape(f, 3 * j)})
    return out


def decided_w(res):
    """|w| of every quaternion whose sign the reference decides: the un-normalised local products of the non-root bodies (quat_pos) and the
    normalised local rotations as_rotvec flips when w < 0 (the root's included)."""
    return np.abs(np.concatenate([res["local_products"][:, 1:, 3].ravel(), res["pose_quat"][..., 3].ravel()]))


def gather(rb, dof_pos, segs):
    """The frames of ``segs`` out of a (T, N, ...) recording, in output order."""
    idx = [(t0 + k, e) for e, t0, n in segs for k in range(n)]
    t, e = [i[0] for i in idx], [i[1] for i in idx]
    return rb[t, e], (None if dof_pos is None else dof_pos[t, e])
