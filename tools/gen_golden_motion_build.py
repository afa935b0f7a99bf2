"""Generate tests/golden/motion_build.npz: what the reference's own loader computes for raw clips, for pulse_motion_build to be held to.

    python tools/gen_golden_motion_build.py [--out DIR]

Needs the reference tree (nothing of its text is kept here: it is read and executed at run time, as oracle/refload.py does).  Per case
the reference's ``MotionLibSMPL.load_motion_with_skeleton`` (phc/utils/motion_lib_smpl.py:101-174, extracted by name: the module
imports smpl_sim) runs on poselib's unmodified ``SkeletonTree`` / ``SkeletonState`` / ``SkeletonMotion`` with
``compute_motion_dof_vels`` / ``local_rotation_to_dof_vel`` (motion_lib_base.py:47-70, extracted by name), mesh_parsers None.
The names the method body looks up are stubbed:

  * ``np.random`` hands out the heading draw the case asks for (angle = pi (2 u - 1)); ``flags.im_eval`` switches the heading off;
  * ``sRot`` is scipy's Rotation, except that ``as_matrix`` comes back in the dtype of the run (torch.matmul wants equal dtypes: the
    reference's data files hold float64 translations) and ``to_torch`` casts to the dtype of the run (scipy hands back float64).

Every case runs twice: in fp32, and with every input promoted to fp64.  The fixture stores the fp32 INPUTS, the fp64 outputs rounded to
fp32, and per field the band  b = max |ref32 - ref64| / max |ref64|  over the whole fixture: the reference's own fp32 error, the only
thing the GPU test's tolerance is made of.  The generator fails unless b <= 1e-4 for every field and every frame-to-frame rotation
angle (global and local) outside the "still" frames lies in [0.02, 2.5] rad: below that acos(2 w^2 - 1) is ill-conditioned in the
reference itself.

Clips: every body's GLOBAL rotation is a steady spin about its own axis (0.08 rad / frame at even tree depth, 0.13 at odd depth, plus
a jitter per body: a body and its parent never turn together) times a small smooth wobble, so both the global and the local
frame-to-frame angles stay inside the band by construction; the root translation drifts and sways; every clip has its own bone offsets.
"""
import argparse
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from pulse_amd import synthetic as syn  # noqa: E402

SEED = 8128
FIELDS = ("gts", "grs", "lrs", "gvs", "gavs", "dvs")
MAX_BYTES = 1 << 20
ANGLE_MIN, ANGLE_MAX, BAND_MAX = 0.02, 2.5, 1e-4

CHAIN33 = [b - 1 for b in range(33)]
STAR64 = [-1] + [0] * 63
# group -> parents, frames per clip, fps per clip, heading angle per clip (None: im_eval, no heading), special
GROUPS = {
    "lengths": dict(parents=syn.SMPL_PARENTS, frames=[2, 3, 8, 9, 16, 17, 18, 40], fps=[30] * 8),
    "smplx": dict(parents=syn.SMPLX_PARENTS, frames=[5, 20], fps=[30, 30]),
    "chain": dict(parents=CHAIN33, frames=[12], fps=[30]),
    "star": dict(parents=STAR64, frames=[12], fps=[30]),
    "fps": dict(parents=syn.SMPL_PARENTS, frames=[10, 10], fps=[30, 60]),
    "heading": dict(parents=syn.SMPL_PARENTS, frames=[10, 10, 10], fps=[30, 30, 30], heading=[2.5, -2.5, 0.0]),
    "still": dict(parents=syn.SMPL_PARENTS, frames=[12], fps=[30], still=(3, 6)),
    "sign": dict(parents=syn.SMPL_PARENTS, frames=[8], fps=[30], negate=((2, None), (5, 7))),     # (frame, body | None = every body)
}


def _quat_exp(v):
    """exp map -> xyzw, float64."""
    ang = np.linalg.norm(v, axis=-1, keepdims=True)
    k = np.where(ang > 1e-12, np.sin(0.5 * ang) / np.maximum(ang, 1e-12), 0.5)
    return np.concatenate([v * k, np.cos(0.5 * ang)], axis=-1)


def _quat_mul(a, b):
    ax, ay, az, aw = np.moveaxis(a, -1, 0)
    bx, by, bz, bw = np.moveaxis(b, -1, 0)
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def _angle(q0, q1):
    """rotation angle between two xyzw rotations, float64, in [0, pi]."""
    d = np.abs(np.sum(q0 * q1, axis=-1)) / (np.linalg.norm(q0, axis=-1) * np.linalg.norm(q1, axis=-1))
    return 2.0 * np.arccos(np.clip(d, 0.0, 1.0))


def make_clip(rng, parents, frames):
    """(rot (F, J, 4) fp32, trans (F, 3) fp32, local_translation (J, 3) fp32) by the recipe of the module docstring."""
    j = len(parents)
    depth = np.zeros(j, dtype=np.int64)
    for b in range(1, j):
        depth[b] = depth[parents[b]] + 1
    t = np.arange(frames, dtype=np.float64)[:, None, None]
    axis = rng.standard_normal((j, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    rate = 0.08 + 0.05 * (depth % 2) + 0.005 * rng.random(j)                                   # rad / frame
    spin = _quat_exp(axis[None] * (rng.random(j)[None, :, None] * 6.2831853 + rate[None, :, None] * t))
    wob = 0.03 * rng.random((j, 3)) * np.sin(0.13 * t + 6.2831853 * rng.random((j, 3)))        # |d wob / frame| <= 0.004 per component
    rot = _quat_mul(_quat_exp(wob), spin)
    rot /= np.linalg.norm(rot, axis=-1, keepdims=True)
    tt = t[:, 0]
    trans = 0.02 * rng.standard_normal(3) * np.array([1.0, 1.0, 0.0]) * tt + 0.05 * rng.standard_normal(3) * np.sin(0.1 * tt) + np.array([0.0, 0.0, 0.9])
    lt = 0.08 + 0.3 * rng.random((j, 3)) * np.array([0.4, 0.4, 1.0])
    lt[0] = 0.0
    return rot.astype(np.float32), trans.astype(np.float32), lt.astype(np.float32)


def cases():
    """group -> dict of fp32 / integer inputs.  Deterministic: one numpy Generator seeded per group."""
    out = {}
    for gi, (name, spec) in enumerate(GROUPS.items()):
        rng = np.random.default_rng(SEED + gi)
        parents = list(spec["parents"])
        clips = [make_clip(rng, parents, f) for f in spec["frames"]]
        rot = np.concatenate([c[0] for c in clips])
        trans = np.concatenate([c[1] for c in clips])
        keep = np.ones(rot.shape[0], dtype=bool)                       # frames whose step to the NEXT frame must satisfy the angle band
        if "still" in spec:
            a, b = spec["still"]
            rot[a:b + 1], trans[a:b + 1] = rot[a], trans[a]
            keep[a:b] = False                                            # steps inside the still stretch: angle exactly 0
        for f, body in spec.get("negate", ()):
            if body is None:
                rot[f] = -rot[f]
            else:
                rot[f, body] = -rot[f, body]
        case = {"rot": rot, "trans": trans, "frames": np.asarray(spec["frames"], dtype=np.int64), "fps": np.asarray(spec["fps"], dtype=np.float32),
                "parents": np.asarray(parents, dtype=np.int32), "local_translation": np.stack([c[2] for c in clips])}
        if "heading" in spec:
            case["heading"] = np.asarray(spec["heading"], dtype=np.float32)
        check_angles(case, keep)
        out[name] = case
    return out


def check_angles(case, keep):
    """Every frame-to-frame rotation angle, global and local (bodies 1 ..), inside [ANGLE_MIN, ANGLE_MAX] except the still steps."""
    rot, par = case["rot"].astype(np.float64), case["parents"]
    conj = rot * np.array([-1.0, -1.0, -1.0, 1.0])
    loc = rot.copy()
    for b in range(1, len(par)):
        loc[:, b] = _quat_mul(conj[:, par[b]], rot[:, b])
    start = 0
    for f in case["frames"]:
        s = slice(start, start + f - 1)
        n = slice(start + 1, start + f)
        for what, q in (("global", rot), ("local", loc[:, 1:])):
            ang = _angle(q[s], q[n])[keep[s]]
            assert ang.size == 0 or (ang.min() >= ANGLE_MIN and ang.max() <= ANGLE_MAX), \
                f"{what} frame-to-frame angle in [{ang.min():.4f}, {ang.max():.4f}] leaves [{ANGLE_MIN}, {ANGLE_MAX}]"
        start += f


# ---------------------------------------------------------------------------------------------------------------- the reference
class _Rot:
    """scipy's Rotation as the method body uses it; as_matrix in the dtype of the run."""

    def __init__(self, r, np_dtype):
        self.r, self.np_dtype = r, np_dtype

    def __mul__(self, other):
        return _Rot(self.r * other.r, self.np_dtype)

    def as_quat(self):
        return self.r.as_quat()

    def as_rotvec(self):
        return self.r.as_rotvec()

    def as_matrix(self):
        return self.r.as_matrix().astype(self.np_dtype)


class _NumpyWithDraws:
    """numpy, with np.random.random() handing out the given draws (np.random.seed / randint: accepted, unused)."""

    def __init__(self, draws):
        draws = list(draws)
        self.random = types.SimpleNamespace(seed=lambda *_: None, randint=lambda *_: 1, random=lambda: draws.pop(0))

    def __getattr__(self, name):
        return getattr(np, name)


def _reference(dtype):
    """load_motion_with_skeleton bound to a namespace for runs in ``dtype``; returns (function, namespace, SkeletonTree)."""
    from scipy.spatial.transform import Rotation
    from oracle import refload
    refload._ensure_paths()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                                           # scipy.ndimage.filters: deprecated namespace
        from poselib.poselib.skeleton.skeleton3d import SkeletonMotion, SkeletonState, SkeletonTree
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    ns = {"torch": torch, "np": np, "torch_utils": refload.torch_utils(), "SkeletonState": SkeletonState, "SkeletonMotion": SkeletonMotion,
          "osp": os.path, "random": __import__("random"), "flags": types.SimpleNamespace(im_eval=False, test=False, real_traj=False),
          "to_torch": lambda x: torch.as_tensor(x).to(dtype),
          "sRot": types.SimpleNamespace(from_euler=lambda *a, **k: _Rot(Rotation.from_euler(*a, **k), np_dtype),
                                        from_quat=lambda q: _Rot(Rotation.from_quat(q), np_dtype),
                                        from_rotvec=lambda v: _Rot(Rotation.from_rotvec(v), np_dtype))}
    base = os.path.join(refload.REFERENCE_ROOT, "phc", "utils")
    srcs = refload._extract(os.path.join(base, "motion_lib_base.py"), ["local_rotation_to_dof_vel", "compute_motion_dof_vels"])
    srcs.update(refload._extract(os.path.join(base, "motion_lib_smpl.py"), ["load_motion_with_skeleton"], methods_of="MotionLibSMPL"))
    for name, text in srcs.items():
        exec(compile(text, f"<reference:{name}>", "exec"), ns)
    return ns["load_motion_with_skeleton"], ns, SkeletonTree


def run_reference(case, dtype):
    """The six tables of one case, clips concatenated, computed by the reference in ``dtype`` -> dict of torch tensors."""
    fn, ns, SkeletonTree = _reference(dtype)
    np_dtype = np.float32 if dtype == torch.float32 else np.float64
    j = len(case["parents"])
    heading = case.get("heading")
    ns["flags"].im_eval = heading is None
    # angle = pi (2 u - 1)  <=>  u = (angle / pi + 1) / 2
    ns["np"] = _NumpyWithDraws([] if heading is None else [(float(h) / math.pi + 1.0) / 2.0 for h in heading])
    data, trees, start = [], [], 0
    for m, f in enumerate(case["frames"]):
        s = slice(start, start + int(f))
        data.append({"pose_quat_global": case["rot"][s].astype(np_dtype), "root_trans_offset": torch.from_numpy(case["trans"][s].astype(np_dtype)),
                     "pose_aa": np.zeros((int(f), j * 3), dtype=np_dtype), "fps": int(case["fps"][m])})
        trees.append(SkeletonTree([str(b) for b in range(j)], torch.from_numpy(case["parents"].astype(np.int32)),
                                  torch.from_numpy(case["local_translation"][m].astype(np_dtype))))
        start += int(f)
    cfg = types.SimpleNamespace(max_length=-1, fix_height=None)
    res = fn(np.arange(len(data)), data, trees, [None] * len(data), None, cfg, None, 0)
    motions = [res[m][1] for m in range(len(data))]
    cat = lambda get: torch.cat([get(mo) for mo in motions], dim=0)                               # motion_lib_base.py:297-304
    return {"gts": cat(lambda mo: mo.global_translation), "grs": cat(lambda mo: mo.global_rotation), "lrs": cat(lambda mo: mo.local_rotation),
            "gvs": cat(lambda mo: mo.global_velocity), "gavs": cat(lambda mo: mo.global_angular_velocity), "dvs": cat(lambda mo: mo.dof_vels)}


def generate(verbose=True):
    cs = cases()
    out = {"groups": np.asarray(list(cs))}
    err = {k: 0.0 for k in FIELDS}
    big = {k: 0.0 for k in FIELDS}
    for name, case in cs.items():
        r32, r64 = run_reference(case, torch.float32), run_reference(case, torch.float64)
        for k, v in case.items():
            out[f"{name}_{k}"] = v
        for k in FIELDS:
            want = r64[k].double()
            assert r32[k].shape == want.shape and torch.isfinite(want).all(), (name, k)
            err[k] = max(err[k], (r32[k].double() - want).abs().max().item())
            big[k] = max(big[k], want.abs().max().item())
            out[f"{name}_{k}_expected"] = want.float().numpy()
    for k in FIELDS:
        band = err[k] / big[k]
        assert band <= BAND_MAX, f"{k}: the reference's own fp32 run is {band:.2e} of the field's largest magnitude from its fp64 run (> {BAND_MAX})"
        out[f"band_{k}"], out[f"max_{k}"] = np.float64(band), np.float64(big[k])
        if verbose:
            print(f"{k:5s} band {band:.3e}   max |ref64| {big[k]:.4f}")
    return out


def write(path):
    np.savez_compressed(path, **generate())
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, f"{path}: {size} bytes > {MAX_BYTES}"
    return size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    path = os.path.join(a.out, "motion_build.npz")
    print(path, write(path), "bytes")


if __name__ == "__main__":
    main()
