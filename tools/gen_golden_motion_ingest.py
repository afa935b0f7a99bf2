"""Generate tests/golden/motion_ingest.npz: what the reference's two conversion scripts compute for raw SMPL clips, for
pulse_motion_ingest to be held to.

    python tools/gen_golden_motion_ingest.py [--out DIR] [--find-seed]

Needs the reference tree and scipy (nothing of the reference's text is kept here: the statements are read and executed at run time, as
oracle/refload.py does).  Per clip the loop bodies of scripts/data_process/convert_amass_data.py (:88-143, from the assignment of ``skip``
to the dict assignment) and convert_amass_isaac.py (:85-138, with ``double`` on: the mirrored copy) run on scipy's Rotation and poselib's
unmodified SkeletonTree / SkeletonState.  Stand-ins only for what smpl_sim supplies: the joint-name lists (pulse_amd/synthetic.py), a
robot object whose calls do nothing, and ``SkeletonTree.from_mjcf`` handing back a tree built from synthetic.SKELETONS["smpl"].

Every clip runs twice: in fp64, and with every array cast to fp32 (``np.zeros`` and ``as_quat`` hand back the dtype of the run: on fp32
inputs the scripts' own zeros and scipy's results would promote everything after them to fp64).  The fixture stores the fp32 INPUTS, the
fp64 outputs, and per field  err = max |ref32 - ref64|  over the whole fixture: the reference's own fp32 error, the only thing the GPU
test's tolerance is made of.  The generator fails unless every quaternion whose sign the reference decides (tests/motion_ingest_model.py:
decided_w) has |w| >= W_FLOOR in the fp64 model: SEED is chosen so that this holds.

Clips (raw frames @ framerate [bound] -> converted frames): 40 @ 120 -> 10, 21 @ 60 -> 11, 37 @ 30 -> 37, 40 @ 100 [2] -> 2 (below the ten
frames convert_amass_data.py:101 asks for: the script drops it, and the fixture holds the isaac script's result for its two frames), 30 @ 30
[13] -> 13.  Clip 0 carries the special rotation vectors: a frame of exact zeros, angles 5e-4, 0.9999e-3, 1.0001e-3, 3.3 and 3.5 (> pi),
6.2 and 6.28 (near 2 pi); every clip has non-zero hand columns.
"""
import argparse
import contextlib
import io
import os
import sys
import textwrap
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import motion_ingest_model as MI  # noqa: E402
from pulse_amd import synthetic as syn  # noqa: E402

SEED = 4243
W_FLOOR = 1e-3
MAX_BYTES = 1 << 20
PATH = os.path.join(ROOT, "tests", "golden", "motion_ingest.npz")
FIELDS = ("pose_quat_global", "pose_quat", "root_trans_offset", "pose_aa", "trans_orig")
MIRROR_FIELDS = ("pose_quat_global", "root_trans_offset")
# raw frames, framerate, bound (0: none)
CLIPS = [(40, 120.0, 0), (21, 60.0, 0), (37, 30.0, 0), (40, 100.0, 2), (30, 30.0, 13)]
ROOT_OFFSET = (0.0013, -0.0021, 0.0257)
# (raw frame, SMPL joint, angle) of clip 0; the frames are multiples of its skip (4), so that they survive the decimation
SPECIAL = [(8, 5, 5e-4), (8, 6, 0.9999e-3), (8, 7, 1.0001e-3), (12, 0, 3.3), (12, 8, 3.5), (12, 9, 6.2), (16, 0, 6.28)]
ZERO_FRAME = 4


def inputs(seed=SEED):
    """The raw clips, fp32: list of dicts {poses (F, 72), trans (F, 3), framerate, bound}."""
    rng = np.random.default_rng(seed)
    out = []
    for ci, (f, rate, bound) in enumerate(CLIPS):
        t = np.arange(f, dtype=np.float64)[:, None, None] / rate
        amp = 0.3 * rng.random((24, 3, 2))
        e = (amp * np.sin(6.2831853 * (0.3 + 1.7 * rng.random((24, 3, 2))) * t[..., None] + 6.2831853 * rng.random((24, 3, 2)))).sum(-1)
        e[:, 0, 2] += 6.2831853 * rng.random() + 0.8 * rng.standard_normal() * t[:, 0, 0]
        tt = t[:, 0]
        trans = 0.6 * rng.standard_normal(3) * np.array([1.0, 1.0, 0.0]) * tt + 0.05 * rng.standard_normal(3) * np.sin(3.0 * tt) + np.array([0.0, 0.0, 0.9])
        if ci == 0:
            e[ZERO_FRAME] = 0.0
            for fr, joint, angle in SPECIAL:
                axis = rng.standard_normal(3)
                e[fr, joint] = axis / np.linalg.norm(axis) * angle
        out.append({"poses": e.reshape(f, 72).astype(np.float32), "trans": trans.astype(np.float32), "framerate": rate, "bound": bound})
    return out


# ---------------------------------------------------------------------------------------------------------------- the reference
def _block(path, first_assigns, last_assigns="amass_full_motion_dict"):
    """The statements of a reference script from the first assignment to ``first_assigns`` to the last one into ``last_assigns[...]``, dedented, run
    once as the body of a one-pass loop (so that ``continue`` leaves it).  Found by the assigned names, as oracle/refload.py finds functions."""
    import re
    with open(path) as f:
        lines = f.read().splitlines()
    first = [i for i, ln in enumerate(lines) if re.match(rf"\s*{first_assigns}\s*=[^=]", ln)]
    last = [i for i, ln in enumerate(lines) if re.match(rf"\s*{last_assigns}\[.*\]\s*=[^=]", ln)]
    assert first and last and first[0] < last[-1], (path, first, last)
    lines = lines[first[0]:last[-1] + 1]
    return "for _once in (0,):\n" + textwrap.indent(textwrap.dedent("\n".join(lines)), "    ")


class _Rot:
    """scipy's Rotation as the scripts use it; as_quat in the dtype of the run."""

    def __init__(self, r, dtype):
        self.r, self.dtype = r, dtype

    def __mul__(self, other):
        return _Rot(self.r * other.r, self.dtype)

    def inv(self):
        return _Rot(self.r.inv(), self.dtype)

    def as_quat(self):
        return self.r.as_quat().astype(self.dtype)


class _Numpy:
    """numpy, with zeros() in the dtype of the run."""

    def __init__(self, dtype):
        self.zeros = lambda shape, *a, **k: np.zeros(shape, dtype=dtype)

    def __getattr__(self, name):
        return getattr(np, name)


class _Log(dict):
    """amass_full_motion_dict: every assignment kept in order (the isaac script stores the mirrored copy under the original's key)."""

    def __init__(self):
        super().__init__()
        self.entries = []

    def __setitem__(self, k, v):
        self.entries.append((k, v))
        super().__setitem__(k, v)


def _namespace(dtype):
    from scipy.spatial.transform import Rotation
    from oracle import refload
    refload._ensure_paths()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from poselib.poselib.skeleton.skeleton3d import SkeletonState, SkeletonTree
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    sk = syn.SKELETONS["smpl"]
    lt = torch.zeros(24, 3, dtype=tdt)
    lt[1:] = torch.linspace(0.05, 0.3, 69, dtype=tdt).reshape(23, 3)           # only local_translation[0] and the parents are read
    lt[0] = torch.tensor(np.asarray(ROOT_OFFSET, dtype=np.float32)).to(tdt)
    tree = SkeletonTree(list(sk["body_names"]), torch.tensor(sk["parents"], dtype=torch.int32), lt)
    robot = types.SimpleNamespace(load_from_skeleton=lambda **k: None, write_xml=lambda *a: None)
    return {"np": _Numpy(dtype), "torch": torch, "SkeletonState": SkeletonState, "SkeletonTree": types.SimpleNamespace(from_mjcf=lambda *a: tree),
            "sRot": types.SimpleNamespace(from_rotvec=lambda v: _Rot(Rotation.from_rotvec(v), dtype), from_quat=lambda q: _Rot(Rotation.from_quat(q), dtype)),
            "smpl_local_robot": robot, "SMPL_BONE_ORDER_NAMES": syn.SMPL_BONE_ORDER_NAMES, "SMPL_MUJOCO_NAMES": syn.SMPL_BODY_NAMES,
            "joint_names": syn.SMPL_BONE_ORDER_NAMES, "mujoco_joint_names": list(syn.SMPL_BODY_NAMES),
            "robot_cfg": {"upright_start": True, "model": "smpl"}, "amass_full_motion_dict": _Log()}


def _arr(v, dtype):
    return (v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(dtype)


def run_reference(clip, dtype):
    """One clip through both scripts in ``dtype`` -> (plain: field -> array, or None where convert_amass_data drops the clip; from the isaac
    script on the decimated frames: plain again, and the mirrored copy)."""
    from oracle import refload
    base = os.path.join(refload.REFERENCE_ROOT, "scripts", "data_process")
    ns = _namespace(dtype)
    ns.update({"framerate": clip["framerate"], "bound": int(clip["bound"]), "key_name_dump": "clip",
               "entry_data": {"trans": clip["trans"].astype(dtype), "poses": clip["poses"].astype(dtype), "betas": np.zeros(16, dtype=dtype),
                              "gender": np.array("neutral")}})
    exec(compile(_block(os.path.join(base, "convert_amass_data.py"), "skip"),
                 "<reference:convert_amass_data>", "exec"), ns)
    plain = {k: _arr(ns["amass_full_motion_dict"]["clip"][k], dtype) for k in FIELDS} if "clip" in ns["amass_full_motion_dict"] else None
    skip, n = MI.decimate(len(clip["poses"]), clip["framerate"], clip["bound"])
    ns = _namespace(dtype)
    ns.update({"pose_aa": clip["poses"].astype(dtype)[::skip][:n].copy(), "root_trans": clip["trans"].astype(dtype)[::skip][:n].copy(), "B": n,
               "beta": np.zeros(16, dtype=dtype), "gender": "neutral", "fps": 30.0, "double": True, "key_name": "clip"})
    with contextlib.redirect_stdout(io.StringIO()):
        exec(compile(_block(os.path.join(base, "convert_amass_isaac.py"), "smpl_2_mujoco"),
                     "<reference:convert_amass_isaac>", "exec"), ns)
    (_, first), (_, second) = ns["amass_full_motion_dict"].entries
    return plain, {k: _arr(first[k], dtype) for k in FIELDS}, {k: _arr(second[k], dtype) for k in FIELDS}


def generate(verbose=True, seed=SEED):
    clips = inputs(seed)
    out = {"num_clips": np.int64(len(clips)), "root_offset": np.asarray(ROOT_OFFSET, dtype=np.float32), "w_floor": np.float64(W_FLOOR)}
    err = {k: 0.0 for k in FIELDS + tuple("mirror_" + k for k in MIRROR_FIELDS)}
    floor = np.inf
    for ci, clip in enumerate(clips):
        p64, i64, m64 = run_reference(clip, np.float64)
        p32, i32, m32 = run_reference(clip, np.float32)
        skip, n = MI.decimate(len(clip["poses"]), clip["framerate"], clip["bound"])
        assert (p64 is None) == (n < MI.MIN_FRAMES) == (p32 is None), ci
        for k in FIELDS:
            assert i64[k].shape[0] == n and (p64 is None or np.array_equal(p64[k], i64[k])), (ci, k)     # the two scripts agree where both run
            assert k in MIRROR_FIELDS or np.array_equal(m64[k], i64[k]), (ci, k)                          # the mirrored copy keeps these
            out[f"c{ci}_{k}"] = i64[k]
            err[k] = max(err[k], float(np.abs(i32[k].astype(np.float64) - i64[k]).max()))
        for k in MIRROR_FIELDS:
            out[f"c{ci}_mirror_{k}"] = m64[k]
            err["mirror_" + k] = max(err["mirror_" + k], float(np.abs(m32[k].astype(np.float64) - m64[k]).max()))
        out[f"c{ci}_poses"], out[f"c{ci}_trans"] = clip["poses"], clip["trans"]
        out[f"c{ci}_framerate"], out[f"c{ci}_bound"], out[f"c{ci}_dropped"] = np.float64(clip["framerate"]), np.int64(clip["bound"]), np.bool_(p64 is None)
        res = MI.ingest_clip(clip["poses"], clip["trans"], clip["framerate"], syn.SMPL_PARENTS, syn.smpl_joint_map(), bound=clip["bound"],
                             root_offset=np.asarray(ROOT_OFFSET, dtype=np.float32))
        floor = min(floor, float(MI.decided_w(res).min()))
    assert floor >= W_FLOOR, f"seed {seed}: a quaternion whose sign is decided has |w| = {floor:.3e} < {W_FLOOR}"
    out["w_min"] = np.float64(floor)
    for k, v in err.items():
        out[f"err_{k}"] = np.float64(v)
        if verbose:
            print(f"{k:28s} max |ref32 - ref64| {v:.3e}")
    if verbose:
        print(f"smallest decided |w| {floor:.3e}")
    return out


def load():
    with np.load(PATH, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def clips_of(fx):
    """The fixture's raw clips as ``inputs`` makes them."""
    return [{"poses": fx[f"c{i}_poses"], "trans": fx[f"c{i}_trans"], "framerate": float(fx[f"c{i}_framerate"]), "bound": int(fx[f"c{i}_bound"])}
            for i in range(int(fx["num_clips"]))]


def find_seed(start=SEED, tries=200):
    for seed in range(start, start + tries):
        w = min(float(MI.decided_w(MI.ingest_clip(c["poses"], c["trans"], c["framerate"], syn.SMPL_PARENTS, syn.smpl_joint_map(), bound=c["bound"])).min())
                for c in inputs(seed))
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
    path = os.path.join(a.out, "motion_ingest.npz")
    np.savez_compressed(path, **generate())
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, f"{path}: {size} bytes > {MAX_BYTES}"
    print(path, size, "bytes")


if __name__ == "__main__":
    main()
