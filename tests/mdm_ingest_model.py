"""A numpy restatement of what pulse_motion_euler_pose and pulse_motion_smooth compute (include/pulse_hip.h section 2b'.1a): the statements of
scripts/data_process/convert_data_mdm.py:48-61 and :128-141 written out -- scipy's from_euler / __mul__ / as_rotvec / as_matrix,
quat_correct as the section defines it, scipy.ndimage's gaussian_filter1d(mode="nearest") and poselib's SkeletonState.local_rotation -- in
fp64, with the intermediate products (raw sign tests, corrected signs, filtered quaternions before the renormalisation) beside the outputs.
The conversion in between (:102-126) is tests/motion_ingest_model.py's.  Needs neither scipy nor a device.

    euler_pose(thetas, trans)              -> pose_aa (F, 72), trans (F, 3)
    smooth_clip(rot, trans, parents, ...)  -> dict: raw_flip, negated (F, J) bool, gap (F - 1, J), corrected, filtered, pose_quat_global,
                                              local_products, pose_quat, root_trans_offset
    mdm_clip(thetas, trans, parents, joint_map, ...) -> euler_pose, then ingest_clip, then smooth_clip: the converted entry
"""
import numpy as np

import motion_ingest_model as MI

FLOOR_HEIGHT = 0.92
ROOT_QUAT = np.array([np.sin(np.pi / 4), 0.0, 0.0, np.cos(np.pi / 4)])     # from_euler('xyz', [pi / 2, 0, 0])
MAX_RADIUS = 12


def quat_matrix(q):
    """scipy Rotation.as_matrix."""
    x, y, z, w = q
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    return np.array([[x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw)], [2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw)],
                     [2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2]])


def as_rotvec(q):
    """scipy Rotation.as_rotvec of quaternions as they are held: w made >= 0, angle = 2 atan2(|xyz|, w), the Taylor branch at angle <= 1e-3."""
    q = np.where(q[..., 3:] < 0, -q, q)
    angle = 2.0 * np.arctan2(np.sqrt((q[..., :3] ** 2).sum(-1)), q[..., 3])
    a2 = angle * angle
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.where(angle <= 1e-3, 2.0 + a2 / 12.0 + 7.0 * a2 * a2 / 2880.0, angle / np.sin(angle / 2.0))
    return scale[..., None] * q[..., :3]


def from_euler_XYZ_degrees(e):
    """Rotation.from_euler('XYZ', e, degrees=True): the elementary quaternions composed left to right (intrinsic); not renormalised."""
    h = np.deg2rad(np.asarray(e, dtype=np.float64)) / 2.0
    z, o = np.zeros_like(h[..., 0]), None
    qx = np.stack([np.sin(h[..., 0]), z, z, np.cos(h[..., 0])], -1)
    qy = np.stack([z, np.sin(h[..., 1]), z, np.cos(h[..., 1])], -1)
    qz = np.stack([z, z, np.sin(h[..., 2]), np.cos(h[..., 2])], -1)
    return MI.scipy_compose(MI.scipy_compose(qx, qy), qz)


def euler_pose(thetas, trans, floor_height=FLOOR_HEIGHT, root_quat=ROOT_QUAT):
    """convert_data_mdm.py:49-59 for one clip."""
    e = np.asarray(thetas, dtype=np.float64).reshape(-1, 24, 3)
    f = e.shape[0]
    aa = as_rotvec(from_euler_XYZ_degrees(e))
    aa[:, 0] = as_rotvec(MI.scipy_unit(MI.scipy_compose(np.asarray(root_quat, dtype=np.float64), MI.from_rotvec(aa[:, 0]))))
    t = np.asarray(trans, dtype=np.float64).dot(quat_matrix(np.asarray(root_quat, dtype=np.float64)).T)
    t[:, 2] = t[:, 2] - (t[0, 2] - floor_height)
    return aa.reshape(f, 72), t


def gaussian_kernel(sigma, radius=None):
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius): the 2 radius + 1 weights."""
    radius = int(4.0 * float(sigma) + 0.5) if radius is None else radius
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def filter_nearest(x, sigma, inner_first=False):
    """gaussian_filter1d(x, sigma, axis=0, mode="nearest"): correlate1d's symmetric branch -- the centre tap, then the pairs from the outermost
    inwards (``inner_first``: the other order, for the summation-order mutation) -- on indices clamped to the array."""
    w = gaussian_kernel(sigma)
    r = len(w) // 2
    n = x.shape[0]
    t = np.arange(n)
    acc = x * w[r]
    for k in (range(1, r + 1) if inner_first else range(r, 0, -1)):
        acc = acc + (x[np.maximum(t - k, 0)] + x[np.minimum(t + k, n - 1)]) * w[r + k]
    return acc


def quat_correct_steps(q):
    """(raw_flip (F, J) bool, gap (F - 1, J)) of (F, J, 4): the test |a - b| > |a + b| between RAW consecutive frames (row 0: False), and
    | |a - b| - |a + b| | of every step."""
    minus = np.linalg.norm(q[:-1] - q[1:], axis=-1)
    plus = np.linalg.norm(q[:-1] + q[1:], axis=-1)
    raw = np.concatenate([np.zeros((1,) + q.shape[1:-1], dtype=bool), minus > plus])
    return raw, np.abs(minus - plus)


def quat_correct(q):
    """The definition (section 2b'.1a): frame t is negated when, against the already corrected frame t - 1, |q[t-1] - q[t]| > |q[t-1] + q[t]|;
    sequentially, one body (F, 4) or many (F, J, 4)."""
    q = q.copy()
    for t in range(1, q.shape[0]):
        flip = np.linalg.norm(q[t - 1] - q[t], axis=-1) > np.linalg.norm(q[t - 1] + q[t], axis=-1)
        q[t] = np.where(flip[..., None], -q[t], q[t])
    return q


def smooth_clip(rot, trans, parents, sigma_rot=2.0, sigma_trans=3.0, inner_first=False):
    """convert_data_mdm.py:131-141 for one clip, as the kernels compute it: the corrected sign as the prefix XOR of the raw tests."""
    rot, trans = np.asarray(rot, dtype=np.float64), np.asarray(trans, dtype=np.float64)
    raw, gap = quat_correct_steps(rot)
    negated = np.logical_xor.accumulate(raw, axis=0)
    corrected = np.where(negated[..., None], -rot, rot)
    if sigma_rot:
        filtered = filter_nearest(corrected, sigma_rot, inner_first)
        glob = filtered / np.linalg.norm(filtered, axis=-1)[..., None]
    else:
        filtered = glob = corrected
    j = len(parents)
    lprod, pq = glob.copy(), glob.copy()
    conj = glob * np.array([-1.0, -1.0, -1.0, 1.0])
    for b in range(1, j):
        lprod[:, b] = MI.quat_mul(conj[:, parents[b]], glob[:, b])
        pq[:, b] = MI.quat_normalize(lprod[:, b])
    pq = pq.astype(np.float32).astype(np.float64)             # poselib collects local rotations in a float32 tensor (motion_ingest_model.py)
    rto = filter_nearest(trans, sigma_trans, inner_first) if sigma_trans else trans
    return {"raw_flip": raw, "negated": negated, "gap": gap, "corrected": corrected, "filtered": filtered, "pose_quat_global": glob,
            "local_products": lprod, "pose_quat": pq, "root_trans_offset": rto}


def mdm_clip(thetas, trans, parents, joint_map, root_offset=(0.0, 0.0, 0.0), floor_height=FLOOR_HEIGHT, sigma_rot=2.0, sigma_trans=3.0, smooth=True):
    """One generated clip through the whole script: the converted entry's fields, and ``ingest`` / ``smooth``: the stages' own dicts."""
    aa, t = euler_pose(thetas, trans, floor_height)
    ing = MI.ingest_clip(aa, t, 30.0, parents, joint_map, root_offset=root_offset)
    out = {"euler_pose": aa, "pose_aa": ing["pose_aa"], "trans_orig": t, "ingest": ing}
    if smooth:
        sm = smooth_clip(ing["pose_quat_global"], ing["root_trans_offset"], parents, sigma_rot, sigma_trans)
        out.update({"smooth": sm, "pose_quat_global": sm["pose_quat_global"], "pose_quat": sm["pose_quat"], "root_trans_offset": sm["root_trans_offset"]})
    else:
        out.update({k: ing[k] for k in ("pose_quat_global", "pose_quat", "root_trans_offset")})
    return out


def sign_words(raw_flip):
    """The 32-bit words of the kernel's first two launches: bit b of word t = body b's raw test, then the prefix XOR along the clip."""
    bits = (raw_flip.astype(np.uint64) << np.arange(raw_flip.shape[1], dtype=np.uint64)).sum(1).astype(np.uint32)
    return bits, np.bitwise_xor.accumulate(bits)
