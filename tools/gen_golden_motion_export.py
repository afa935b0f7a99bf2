"""Generate tests/golden/motion_export.npz: what the reference computes from a recorded rollout, for pulse_motion_export to be held to.

    python tools/gen_golden_motion_export.py [--out DIR] [--find-seed]

Needs the reference tree, scipy and poselib (nothing of the reference's text is kept here: the statements are read and executed at run time, as
oracle/refload.py and tools/gen_golden_motion_ingest.py do):
  * the conversion lines of HumanoidIm.render's upright branch (phc/env/tasks/humanoid_im.py, from the assignment of ``N`` to the one of the
    permuted ``pose_aa``) and the line that builds ``mujoco_2_smpl``, on scipy's Rotation and poselib's unmodified SkeletonState;
  * the body of Humanoid._write_states_to_file (phc/env/tasks/humanoid.py) with ``joblib.dump`` captured;
  * the round trip: the loop body of scripts/data_process/convert_amass_isaac.py on the pose_aa / trans the render chain gave.
Stand-ins only for what the simulator and the GPU supply: a ``self`` that carries the recording, ``Tensor.cuda`` handing back the tensor.

Every chain runs twice: in fp64, and with every stage boundary cast to fp32 (``as_quat`` / ``as_rotvec`` hand back the dtype of the run).  The
fixture stores the fp32 INPUTS, the fp64 outputs, and per field  err = max |ref32 - ref64|  over the fixture: the reference's own fp32 error,
the only thing the GPU test's tolerance is made of.  The generator fails unless every quaternion whose sign the reference decides
(tests/motion_export_model.py: decided_w) has |w| >= W_FLOOR in the fp64 model: SEED is chosen so that this holds.

The recording: T = 7 steps x N = 9 envs x 24 bodies = 63 frames (7.875 workgroups of eight frames; 8 idle lanes per half-wave), PROGRESS below:
an env that never resets, 1-frame segments, a reset that moves progress by exactly 1 (no split), a split at the last step.  Special local
rotations (SPECIAL: step, env, SMPL joint): exact identity, angles 5e-4, 0.9999e-3, 1.0001e-3 (realised within ANGLE_WINDOW after the fp32
rounding of the global rotations: the generator searches the requested angle), 3.0; global quaternions stored as -q (w < 0) and scaled to
norm 1 +- 1e-6.  The hand joints (SMPL 22, 23) are identity on the round-trip frames (envs < ROUNDTRIP_ENVS): ingest zeroes them.
"""
import argparse
import contextlib
import io
import os
import re
import sys
import textwrap
import types
from collections import defaultdict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden_motion_ingest as GI  # noqa: E402
import motion_export_model as MX  # noqa: E402
import motion_ingest_model as MI  # noqa: E402
from pulse_amd import synthetic as syn  # noqa: E402

SEED = 7301
W_FLOOR = 1e-3
MAX_BYTES = 1 << 20
PATH = os.path.join(ROOT, "tests", "golden", "motion_export.npz")
T, N, J = 7, 9, 24
ROOT_OFFSET = GI.ROOT_OFFSET
ROUNDTRIP_ENVS = 6
PROGRESS = [[5, 6, 7, 8, 9, 10, 11],          # never resets: one 7-frame segment
            [20, 21, 22, 0, 10, 11, 12],      # a 1-frame segment in the middle
            [0, 1, 0, 1, 2, 3, 4],            # a reset that moves progress by exactly 1: no split
            [3, 4, 5, 6, 7, 8, 0],            # a split at the last step
            [30, 0, 1, 2, 3, 4, 5],           # a 1-frame segment at the start
            [0, 1, 2, 3, 0, 1, 2],
            [9, 10, 11, 12, 13, 0, 1],
            [2, 3, 4, 5, 6, 7, 8],
            [4, 0, 4, 0, 4, 0, 4]]            # seven 1-frame segments
SEGMENT_FRAMES = [7, 3, 1, 3, 7, 6, 1, 1, 6, 4, 3, 5, 2, 7, 1, 1, 1, 1, 1, 1, 1]
# (step, env, SMPL joint, angle); None: exact identity
SPECIAL = [(1, 0, 5, None), (2, 0, 5, 5e-4), (2, 0, 6, 0.9999e-3), (2, 0, 7, 1.0001e-3), (3, 0, 8, 3.0), (3, 1, 0, 3.0)]
ANGLE_WINDOW = {5e-4: (4.9995e-4, 5.0005e-4), 0.9999e-3: (0.99985e-3, 0.99995e-3), 1.0001e-3: (1.00005e-3, 1.00015e-3), 3.0: (2.99999, 3.00001)}
NEGATED = [(4, 0, 0), (4, 0, 7), (4, 7, 11)]                 # (step, env, BODY): the global quaternion stored as -q
SCALED = [(5, 0, 3, 1.0 + 1e-6), (5, 0, 4, 1.0 - 1e-6)]      # (step, env, BODY, norm)
DOF_SPECIAL = [(0, 0, 2, 0.0), (0, 0, 3, 4.0), (0, 0, 4, 5e-6), (1, 3, 9, 3.1)]     # (step, env, joint 0 .. 22, |exp map|): the default axis, > pi, masked
FIELDS = ("pose_quat_global", "root_trans_offset", "pose_quat", "pose_aa", "trans_orig")
STATE_FIELDS = ("body_quat", "trans", "root_states_seg", "dof_pos")


# ---------------------------------------------------------------------------------------------------------------- the inputs
def sim_rotations(pose_aa):
    """The simulator's global body rotations (fp64) of SMPL poses (F, 24, 3): the ingest direction, hands kept."""
    parents, jm = syn.SMPL_PARENTS, syn.smpl_joint_map()
    local = MI.from_rotvec(pose_aa[:, jm])
    glob = local.copy()
    for b in range(1, J):
        glob[:, b] = MI.quat_normalize(MI.quat_mul(glob[:, parents[b]], local[:, b]))
    return MI.scipy_unit(MI.scipy_compose(MI.scipy_unit(glob), np.array([-0.5, -0.5, -0.5, 0.5])))


def _realised(pose_aa_frame):
    """Angles (24, SMPL joint order) the fp64 chain finds in the fp32 rotations of one frame."""
    rb = np.zeros((1, J, 13), dtype=np.float32)
    rb[0, :, 3:7] = sim_rotations(pose_aa_frame[None]).astype(np.float32)[0]
    aa = MX.export_frames(rb, None, syn.SMPL_PARENTS, syn.smpl_joint_map())["pose_aa"]
    return np.linalg.norm(aa.reshape(J, 3), axis=-1)


def inputs(seed=SEED):
    """-> rb (T, N, 24, 13) fp32, dof_pos (T, N, 69) fp32, progress (T, N) int64."""
    rng = np.random.default_rng(seed)
    aa = rng.standard_normal((T, N, J, 3))
    aa = aa / np.linalg.norm(aa, axis=-1, keepdims=True) * (0.05 + 0.75 * rng.random((T, N, J, 1)))
    root = rng.standard_normal((T, N, 3))
    aa[:, :, 0] = root / np.linalg.norm(root, axis=-1, keepdims=True) * (0.5 + 2.0 * rng.random((T, N, 1)))
    aa[:, :ROUNDTRIP_ENVS, 22:] = 0.0
    for t, e, s, angle in SPECIAL:
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        if angle is None:
            aa[t, e, s] = 0.0
            continue
        lo, hi = ANGLE_WINDOW[angle]
        for k in range(2000):                                 # the fp32 rounding of the globals moves a small angle by ~1e-7: search the request
            aa[t, e, s] = axis * (angle + (k // 2) * (1 if k % 2 else -1) * 1e-9 * (angle / 1e-3))
            if lo < _realised(aa[t, e])[s] < hi:
                break
        else:
            raise RuntimeError(f"seed {seed}: no request realises angle {angle} at {(t, e, s)}")
    rb = np.zeros((T, N, J, 13), dtype=np.float32)
    rot = sim_rotations(aa.reshape(T * N, J, 3)).astype(np.float32).reshape(T, N, J, 4)
    for t, e, s, angle in SPECIAL:
        if angle is None:                                     # exact identity: the child's global rotation IS its parent's
            b = syn.smpl_joint_map().index(s)
            rot[t, e, b] = rot[t, e, syn.SMPL_PARENTS[b]]
    for t, e, b in NEGATED:
        rot[t, e, b] = -rot[t, e, b]
    for t, e, b, norm in SCALED:
        rot[t, e, b] = (rot[t, e, b].astype(np.float64) * norm).astype(np.float32)
    rb[..., 3:7] = rot
    rb[..., 0, 0:3] = (rng.standard_normal((T, N, 3)) * np.array([2.0, 2.0, 0.05]) + np.array([0.0, 0.0, 0.9])).astype(np.float32)
    rb[..., 1:, 0:3] = rb[..., :1, 0:3] + 0.3 * rng.standard_normal((T, N, J - 1, 3)).astype(np.float32)
    rb[..., 7:13] = rng.standard_normal((T, N, J, 6)).astype(np.float32)
    dof = rng.standard_normal((T, N, J - 1, 3))
    dof = dof / np.linalg.norm(dof, axis=-1, keepdims=True) * (0.1 + 1.4 * rng.random((T, N, J - 1, 1)))
    for t, e, j, mag in DOF_SPECIAL:                         # (the masked one along x: its other components are exact zeros, not small numbers)
        dof[t, e, j] = dof[t, e, j] / np.linalg.norm(dof[t, e, j]) * mag if mag > 1e-5 else np.array([mag, 0.0, 0.0])
    return rb, dof.reshape(T, N, 3 * (J - 1)).astype(np.float32), np.asarray(PROGRESS, dtype=np.int64).T.copy()


# ---------------------------------------------------------------------------------------------------------------- the reference
class _Rot(GI._Rot):
    def as_rotvec(self):
        return self.r.as_rotvec().astype(self.dtype)


def _srot(dtype):
    from scipy.spatial.transform import Rotation
    return types.SimpleNamespace(from_quat=lambda q: _Rot(Rotation.from_quat(np.asarray(q)), dtype), identity=lambda: _Rot(Rotation.identity(), dtype))


@contextlib.contextmanager
def _cuda_is_here():
    keep = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.Tensor.cuda = keep


def _lines(path, first, last, after=None):
    """The statements of a reference file from the first line matching ``first`` (after the first one matching ``after``) to the next one matching
    ``last``, dedented."""
    with open(path) as f:
        lines = f.read().splitlines()
    at = next(i for i, ln in enumerate(lines) if re.match(after, ln)) if after else 0
    a = next(i for i in range(at, len(lines)) if re.match(first, lines[i]))
    b = next(i for i in range(a, len(lines)) if re.match(last, lines[i]))
    return textwrap.dedent("\n".join(lines[a:b + 1]))


def run_render(rot, root_pos, dtype):
    """render()'s upright conversion of F frames at once -> upright globals, pose_quat, pose_aa (F, 72), trans_orig, in ``dtype``."""
    from oracle import refload
    path = os.path.join(refload.REFERENCE_ROOT, "phc", "env", "tasks", "humanoid_im.py")
    ns = GI._namespace(dtype)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    srot = _srot(dtype)
    me = types.SimpleNamespace(_body_names_orig=list(syn.SMPL_BODY_NAMES), skeleton_trees=[ns["SkeletonTree"].from_mjcf()], pre_rot=srot.from_quat([0.5, 0.5, 0.5, 0.5]))
    env = {"self": me, "sRot": srot, "SkeletonState": ns["SkeletonState"], "torch": torch, "np": np, "SMPL_BONE_ORDER_NAMES": syn.SMPL_BONE_ORDER_NAMES,
           "body_quat": torch.from_numpy(rot.astype(dtype)), "root_trans": torch.from_numpy(root_pos.astype(dtype))}
    assert env["body_quat"].dtype == tdt
    exec(compile(_lines(path, r"\s*self\.mujoco_2_smpl\s*=", r"\s*self\.mujoco_2_smpl\s*="), "<reference:humanoid_im mujoco_2_smpl>", "exec"), env)
    with _cuda_is_here():
        exec(compile(_lines(path, r"\s*N\s*=\s*body_quat", r"\s*pose_aa\s*=\s*torch\.from_numpy", after=r"\s*def render\("), "<reference:humanoid_im render>", "exec"), env)
    return {"upright": GI._arr(env["pose_quat"], dtype), "pose_quat": GI._arr(env["local_rot"], dtype), "pose_aa": GI._arr(env["pose_aa"], dtype),
            "trans_orig": GI._arr(env["root_trans_offset"], dtype), "mujoco_2_smpl": [int(v) for v in me.mujoco_2_smpl]}


def run_write_states(rb, dof_pos, progress, dtype):
    """The body of _write_states_to_file on the recording -> the dict it hands to joblib.dump (key -> field -> array)."""
    from oracle import refload
    path = os.path.join(refload.REFERENCE_ROOT, "phc", "env", "tasks", "humanoid.py")
    src = refload._extract(path, ["_write_states_to_file"], methods_of="Humanoid")["_write_states_to_file"]
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    dumped = {}
    ns = {"torch": torch, "torch_utils": refload.torch_utils(), "defaultdict": defaultdict,
          "joblib": types.SimpleNamespace(dump=lambda obj, name: dumped.update(obj))}
    exec(compile(src, "<reference:humanoid _write_states_to_file>", "exec"), ns)
    record = defaultdict(list)
    for t in range(rb.shape[0]):
        record["dof_pos"].append(torch.from_numpy(dof_pos[t]).to(tdt))
        record["root_states"].append(torch.from_numpy(rb[t, :, 0]).to(tdt))
        record["progress"].append(torch.from_numpy(progress[t]))
    me = types.SimpleNamespace(state_record=record, skeleton_trees=[types.SimpleNamespace(to_dict=lambda i=i: {"slot": i}) for i in range(rb.shape[1])],
                               humanoid_shapes=torch.arange(rb.shape[1] * 17, dtype=torch.float32).reshape(-1, 17))
    with contextlib.redirect_stdout(io.StringIO()):
        ns["_write_states_to_file"](me, "states.pkl")
    return {str(k): {f: (GI._arr(v[f], dtype) if f in STATE_FIELDS else v[f]) for f in v} for k, v in dumped.items()}


def run_isaac(pose_aa, trans, dtype):
    """The loop body of convert_amass_isaac.py on (F, 72) pose_aa / (F, 3) trans -> pose_quat_global, root_trans_offset."""
    from oracle import refload
    ns = GI._namespace(dtype)
    ns.update({"pose_aa": pose_aa.astype(dtype).copy(), "root_trans": trans.astype(dtype).copy(), "B": pose_aa.shape[0], "beta": np.zeros(16, dtype=dtype),
               "gender": "neutral", "fps": 30.0, "double": False, "key_name": "clip"})
    with contextlib.redirect_stdout(io.StringIO()):
        exec(compile(GI._block(os.path.join(refload.REFERENCE_ROOT, "scripts", "data_process", "convert_amass_isaac.py"), "smpl_2_mujoco"),
                     "<reference:convert_amass_isaac>", "exec"), ns)
    first = ns["amass_full_motion_dict"].entries[0][1]
    return {k: GI._arr(first[k], dtype) for k in ("pose_quat_global", "root_trans_offset")}


def generate(verbose=True, seed=SEED):
    rb, dof, progress = inputs(seed)
    segs = MX.segments(progress)
    frames, dofs = MX.gather(rb, dof, segs)                                   # output order: env-major, then time
    out = {"rb": rb, "dof_pos": dof, "progress": progress, "root_offset": np.asarray(ROOT_OFFSET, dtype=np.float32), "w_floor": np.float64(W_FLOOR),
           "seg_env": np.array([s[0] for s in segs]), "seg_t0": np.array([s[1] for s in segs]), "seg_frames": np.array([s[2] for s in segs])}
    run = {dt: run_render(frames[:, :, 3:7], frames[:, 0, 0:3], dt) for dt in (np.float64, np.float32)}
    r64, r32 = run[np.float64], run[np.float32]
    assert r64["mujoco_2_smpl"] == [syn.smpl_joint_map().index(s) for s in range(J)]
    ref64 = {"pose_quat_global": frames[:, :, 3:7].astype(np.float64), "root_trans_offset": frames[:, 0, 0:3].astype(np.float64), "pose_quat": r64["pose_quat"],
             "pose_aa": r64["pose_aa"], "trans_orig": r64["trans_orig"]}
    ref32 = {"pose_quat_global": frames[:, :, 3:7], "root_trans_offset": frames[:, 0, 0:3], "pose_quat": r32["pose_quat"], "pose_aa": r32["pose_aa"],
             "trans_orig": r32["trans_orig"]}
    err = {}
    for k in FIELDS:
        out[k] = ref64[k]
        err[k] = float(np.abs(ref32[k].astype(np.float64) - ref64[k]).max())
    # the dump
    s64, s32 = run_write_states(rb, dof, progress, np.float64), run_write_states(rb, dof, progress, np.float32)
    keys = MX.segment_keys(segs)
    assert list(s64) == keys == list(s32), (list(s64), keys)
    out["keys"] = np.array(keys)
    for f in STATE_FIELDS:
        out["states_" + f] = np.concatenate([s64[k][f] for k in keys])
        err["states_" + f] = float(np.abs(np.concatenate([s32[k][f] for k in keys]).astype(np.float64) - out["states_" + f]).max())
    assert all(s64[k]["fps"] == 60 for k in keys)
    # the round trip, on the frames whose hands are identity
    sel = np.array([i for i, e in enumerate(s[0] for s in segs for _ in range(s[2])) if e < ROUNDTRIP_ENVS])
    out["roundtrip_frames"] = sel
    t64 = run_isaac(r64["pose_aa"][sel], r64["trans_orig"][sel], np.float64)
    t32 = run_isaac(r32["pose_aa"][sel], r32["trans_orig"][sel], np.float32)
    for k in ("pose_quat_global", "root_trans_offset"):
        out["roundtrip_" + k] = t64[k]
        err["roundtrip_" + k] = float(np.abs(t32[k].astype(np.float64) - t64[k]).max())
    res = MX.export_frames(frames, dofs, syn.SMPL_PARENTS, syn.smpl_joint_map(), root_offset=out["root_offset"])
    floor = float(MX.decided_w(res).min())
    assert floor >= W_FLOOR, f"seed {seed}: a quaternion whose sign is decided has |w| = {floor:.3e} < {W_FLOOR}"
    out["w_min"] = np.float64(floor)
    for k, v in err.items():
        out[f"err_{k}"] = np.float64(v)
        if verbose:
            print(f"{k:32s} max |ref32 - ref64| {v:.3e}")
    if verbose:
        print(f"smallest decided |w| {floor:.3e}; {len(segs)} segments, {len(frames)} frames, {len(sel)} round-trip frames")
    return out


def load():
    with np.load(PATH, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def segs_of(fx):
    return list(zip(fx["seg_env"].tolist(), fx["seg_t0"].tolist(), fx["seg_frames"].tolist()))


def find_seed(start=SEED, tries=200):
    for seed in range(start, start + tries):
        rb, dof, progress = inputs(seed)
        frames, dofs = MX.gather(rb, dof, MX.segments(progress))
        w = float(MX.decided_w(MX.export_frames(frames, dofs, syn.SMPL_PARENTS, syn.smpl_joint_map())).min())
        if w >= W_FLOOR:
            return seed, w
    raise RuntimeError("no seed found")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.dirname(PATH))
    ap.add_argument("--find-seed", action="store_true")
    a = ap.parse_args()
    if a.find_seed:
        print(find_seed())
        return
    path = os.path.join(a.out, "motion_export.npz")
    np.savez_compressed(path, **generate())
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, f"{path}: {size} bytes > {MAX_BYTES}"
    print(path, size, "bytes")


if __name__ == "__main__":
    main()
