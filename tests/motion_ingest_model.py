"""A numpy restatement of what pulse_motion_ingest computes (include/pulse_hip.h section 2b'.1): the statements of
scripts/data_process/convert_amass_isaac.py:85-137 and convert_amass_data.py:88-141 written out -- scipy's from_rotvec / from_quat /
__mul__ / inv and poselib's quat_mul_norm / SkeletonState.global_rotation / local_rotation -- in fp64 by default, and every intermediate
product handed back beside the outputs, so that a test can look at the quaternions whose SIGN the reference decides (quat_pos, w < 0).

    ingest_clip(poses, trans, ...) -> dict
      pose_aa (N, 3 S), trans_orig (N, 3), pose_local (N, J, 4) from_rotvec, global_products (N, J, 4) the un-normalised quat_mul of every
      non-root body (root row: the root itself), global (N, J, 4), pose_quat_global (N, J, 4), local_products (N, J, 4), pose_quat (N, J, 4),
      root_trans_offset (N, 3)
"""
import numpy as np

# SMPL's joint order under the names the humanoid's bodies carry (the public SMPL kinematic tree)
SMPL_JOINTS = 24
HAND_COL = 66
MIN_FRAMES = 10


def decimate(num_frames, framerate, bound=None):
    """(skip, kept frames): skip = int(framerate / 30), frames [::skip][:bound] (convert_amass_data.py:88-100)."""
    skip = int(framerate / 30)
    if skip < 1:
        raise ValueError(f"framerate {framerate}: int(framerate / 30) is 0")
    n = -(-num_frames // skip)
    return skip, (n if not bound else min(n, int(bound)))


def quat_mul(a, b):
    """poselib rotation3d.quat_mul (:15-27)."""
    x1, y1, z1, w1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    x2, y2, z2, w2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    w = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2
    x = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2
    y = w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2
    z = w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2
    return np.stack([x, y, z, w], axis=-1)


def quat_normalize(q):
    """quat_unit(quat_pos(q)) (:31-38, 51-56, 93-98)."""
    one = q.dtype.type(1)
    q = np.where(q[..., 3:] < 0, -one, one) * q
    n = np.sqrt((q * q).sum(-1, keepdims=True))
    return q / np.maximum(n, q.dtype.type(1e-9))


def from_rotvec(v):
    """scipy Rotation.from_rotvec: xyzw, the Taylor branch at angle <= 1e-3, w as cos gives it."""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    angle = np.sqrt(x * x + y * y + z * z)
    t = v.dtype.type
    a2 = angle * angle
    small = t(0.5) - a2 / t(48) + a2 * a2 / t(3840)
    with np.errstate(invalid="ignore", divide="ignore"):
        large = np.sin(angle / t(2)) / angle
    scale = np.where(angle.astype(np.float64) <= 1e-3, small, large)
    return np.concatenate([scale[..., None] * v, np.cos(angle / t(2))[..., None]], axis=-1)


def scipy_unit(q):
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def scipy_compose(p, q):
    """scipy _compose_quat: the product, the sign kept."""
    cx = p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1]
    cy = p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2]
    cz = p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]
    return np.stack([p[..., 3] * q[..., 0] + q[..., 3] * p[..., 0] + cx, p[..., 3] * q[..., 1] + q[..., 3] * p[..., 1] + cy,
                     p[..., 3] * q[..., 2] + q[..., 3] * p[..., 2] + cz,
                     p[..., 3] * q[..., 3] - p[..., 0] * q[..., 0] - p[..., 1] * q[..., 1] - p[..., 2] * q[..., 2]], axis=-1)


def ingest_clip(poses, trans, framerate, parents, joint_map, *, bound=None, upright_start=True, mirror=False, mirror_map=None,
                root_offset=(0.0, 0.0, 0.0), dtype=np.float64):
    skip, n = decimate(len(poses), framerate, bound)
    poses, trans = np.asarray(poses, dtype=dtype)[::skip][:n], np.asarray(trans, dtype=dtype)[::skip][:n]
    s = poses.shape[1] // 3
    pose_aa = np.concatenate([poses[:, :HAND_COL], np.zeros((n, 3 * s - HAND_COL), dtype=dtype)], axis=1)
    local = from_rotvec(pose_aa.reshape(n, s, 3)[:, list(joint_map)])
    j = len(parents)
    gprod, glob = local.copy(), local.copy()
    for b in range(1, j):
        gprod[:, b] = quat_mul(glob[:, parents[b]], local[:, b])
        glob[:, b] = quat_normalize(gprod[:, b])
    out = {"pose_aa": pose_aa, "trans_orig": trans, "pose_local": local, "global_products": gprod, "global": glob}
    if upright_start:
        inv = np.array([-0.5, -0.5, -0.5, 0.5], dtype=dtype)
        pqg = scipy_unit(scipy_compose(scipy_unit(glob), inv))
        lprod, pq = pqg.copy(), pqg.copy()
        conj = pqg * np.array([-1, -1, -1, 1], dtype=dtype)
        for b in range(1, j):
            lprod[:, b] = quat_mul(conj[:, parents[b]], pqg[:, b])
            pq[:, b] = quat_normalize(lprod[:, b])
        # poselib collects the local rotations in quat_identity_like(...), a float32 tensor whatever the dtype of the state (rotation3d.py:112-119,
        # skeleton3d.py:449): the reference's pose_quat is rounded to fp32 even where everything before it ran in fp64
        pq = pq.astype(np.float32).astype(dtype)
    else:
        pqg, lprod, pq = glob, local.copy(), local
    rto = trans + np.asarray(root_offset, dtype=dtype)
    if mirror:
        pqg = pqg[:, list(mirror_map)] * np.array([-1, 1, -1, 1], dtype=dtype)
        rto = rto * np.array([1, -1, 1], dtype=dtype)
    out.update({"pose_quat_global": pqg, "local_products": lprod, "pose_quat": pq, "root_trans_offset": rto})
    return out


def decided_w(res):
    """|w| of every quaternion whose sign quat_pos decides: the un-normalised products of the non-root bodies, down the tree and back."""
    return np.abs(np.concatenate([res["global_products"][:, 1:, 3].ravel(), res["local_products"][:, 1:, 3].ravel()]))
