"""Generate tests/golden/mdm_ingest.npz: what the reference's scripts/data_process/convert_data_mdm.py computes for generated (text-to-motion)
clips, for pulse_motion_euler_pose, pulse_motion_ingest and pulse_motion_smooth to be held to.

    python tools/gen_golden_mdm_ingest.py [--out DIR] [--find-seed]

Needs the reference tree and scipy (nothing of the reference's text is kept here: the statements are read and executed at run time, as
tools/gen_golden_motion_ingest.py does, whose stand-ins this tool reuses).  Per clip the body of the script's first loop (:49-61, from the
assignment of ``pose_euler`` to the one into ``amass_data``) and of its second (:68-152, from ``key_name_dump`` to the one into
``amass_full_motion_dict``) run on scipy's Rotation, scipy.ndimage's gaussian_filter1d and poselib's unmodified SkeletonState.  Stand-ins only
for what smpl_sim supplies: the joint-name lists, a robot object whose calls do nothing, ``SkeletonTree.from_mjcf`` handing back a tree built
from synthetic.SKELETONS["smpl"], and ``quat_correct`` (third-party, absent): the definition of include/pulse_hip.h section 2b'.1a -- frame t
is negated when, against the already corrected frame t - 1, |q[t-1] - q[t]| > |q[t-1] + q[t]| -- the criterion the script's own line :135 states.

Every clip runs twice: in fp64, and with every array cast to fp32 (``np.zeros`` and scipy's as_quat / as_rotvec / as_matrix hand back the dtype
of the run).  The fixture stores the fp32 INPUTS, the fp64 outputs, and per field  err = max |ref32 - ref64|  over the whole fixture.

Clips: 10, 11, 26 and 65 frames (112 together).  SEED is chosen (``--find-seed``, on tests/mdm_ingest_model.py) so that ``conditions`` holds;
the generator checks it again on the reference's own arrays and fails otherwise:
  * every raw step of every body has | |a - b| - |a + b| | >= GAP_FLOOR, far above ``margin`` (below), so that no fp32 evaluation decides a sign
    differently;
  * a negation at frame 1 of a clip; a negated last frame of a clip; two sign changes of one body within 8 frames; a body of the 65-frame clip
    whose sign is negative at frame 63, where the scan's 64-frame step hands its carry on; a body of a clip that is never negated;
  * no filtered quaternion with a norm below 0.5 before the renormalisation;
  * every quaternion whose sign quat_pos decides (the conversion's products and the local rotations of the filtered globals) has |w| >= W_FLOOR.
margin = 2 (2 (8 e + 2^-23) + 2^-21) with e = err_pose_quat_global of tests/golden/motion_ingest.npz's kind, here taken as 1e-6: a kernel held to
4 e per component hands the sign test quaternions whose sums and differences are off by at most 8 e + 2^-23 per component, a 4-vector's norm by
at most twice that, the fp32 evaluation of a norm <= 2 adds at most 2^-21, and two norms are compared.
"""
import argparse
import contextlib
import io
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden_motion_ingest as GI  # noqa: E402
import mdm_ingest_model as MM  # noqa: E402
import motion_ingest_model as MI  # noqa: E402
from pulse_amd import synthetic as syn  # noqa: E402

SEED = 7009
W_FLOOR = 1e-3
GAP_FLOOR = 1e-2
MARGIN = 2.0 * (2.0 * (8.0 * 1e-6 + 2.0 ** -23) + 2.0 ** -21)
MAX_BYTES = 1 << 20
PATH = os.path.join(ROOT, "tests", "golden", "mdm_ingest.npz")
FIELDS = GI.FIELDS
FRAMES = (10, 11, 26, 65)
ROOT_OFFSET = GI.ROOT_OFFSET


def inputs(seed=SEED):
    """The generated clips, fp32: list of dicts {thetas (F, 24, 3) degrees, root_translation (F, 3)}."""
    rng = np.random.default_rng(seed)
    out = []
    for f in FRAMES:
        t = np.arange(f, dtype=np.float64)[:, None, None]
        amp = 12.0 * rng.random((24, 3, 2))
        e = (amp * np.sin(6.2831853 * (0.01 + 0.05 * rng.random((24, 3, 2))) * t[..., None] + 6.2831853 * rng.random((24, 3, 2)))).sum(-1)
        e[:, 0, 1] += 360.0 * rng.random() + rng.uniform(-25.0, 25.0) * t[:, 0, 0]                 # the root turns about the vertical (y, before :54)
        for joint in rng.choice(np.arange(1, 22), 3, replace=False):                                # three limbs swing around a half turn
            e[:, joint, rng.integers(3)] += 180.0 + 40.0 * np.sin(6.2831853 * t[:, 0, 0] / rng.uniform(6.0, 14.0) + 6.2831853 * rng.random())
        e += 1.5 * rng.standard_normal(e.shape)                                                     # jitter
        tt = t[:, 0] / 30.0
        trans = 0.6 * rng.standard_normal(3) * np.array([1.0, 0.0, 1.0]) * tt + 0.05 * rng.standard_normal(3) * np.sin(3.0 * tt) + np.array([0.0, 0.9, 0.0])
        trans += 0.004 * rng.standard_normal(trans.shape)
        out.append({"thetas": e.astype(np.float32), "root_translation": trans.astype(np.float32)})
    return out


def model(clip):
    return MM.mdm_clip(clip["thetas"], clip["root_translation"], syn.SMPL_PARENTS, syn.smpl_joint_map(), root_offset=np.asarray(ROOT_OFFSET, dtype=np.float32))


def conditions(stages):
    """The fixture conditions (module docstring) on per-clip dicts {raw_flip, negated (F, J), gap (F - 1, J), filtered (F, J, 4), decided_w (...)}:
    name -> bool, and the figures."""
    gap = min(float(s["gap"].min()) for s in stages)
    norm = min(float(np.linalg.norm(s["filtered"], axis=-1).min()) for s in stages)
    w = min(float(s["decided_w"].min()) for s in stages)
    twice = False
    for s in stages:
        for b in range(s["raw_flip"].shape[1]):
            at = np.flatnonzero(s["raw_flip"][:, b])
            twice = twice or bool(len(at) > 1 and np.diff(at).min() <= 8)
    long = [s for s in stages if s["negated"].shape[0] > 64]
    ok = {"gap": gap >= GAP_FLOOR and gap > MARGIN, "frame_1": any(s["negated"][1].any() for s in stages), "last_frame": any(s["negated"][-1].any() for s in stages),
          "twice_in_8": twice, "carry_at_64": any(s["negated"][63].any() for s in long), "never": any((~s["negated"].any(0)).any() for s in stages),
          "norm": norm >= 0.5, "decided_w": w >= W_FLOOR}
    return ok, {"gap_min": gap, "norm_min": norm, "w_min": w}


def stage_of(res):
    """``conditions``' input from tests/mdm_ingest_model.py's result of one clip."""
    sm = res["smooth"]
    return {"raw_flip": sm["raw_flip"], "negated": sm["negated"], "gap": sm["gap"], "filtered": sm["filtered"],
            "decided_w": np.concatenate([MI.decided_w(res["ingest"]), np.abs(sm["local_products"][:, 1:, 3]).ravel()])}


# ---------------------------------------------------------------------------------------------------------------- the reference
class _Rot(GI._Rot):
    def __mul__(self, other):
        return _Rot(self.r * other.r, self.dtype)

    def as_rotvec(self):
        return self.r.as_rotvec().astype(self.dtype)

    def as_matrix(self):
        return self.r.as_matrix().astype(self.dtype)


def _quat_correct(quat):
    """The stand-in for smpl_sim.utils.transform_utils.quat_correct: the definition (module docstring), in the dtype of its input."""
    quat = quat.copy()
    for t in range(1, quat.shape[0]):
        if np.linalg.norm(quat[t - 1] - quat[t]) > np.linalg.norm(quat[t - 1] + quat[t]):
            quat[t] = -quat[t]
    return quat


@contextlib.contextmanager
def _smpl_sim_stand_in():
    names = ("smpl_sim", "smpl_sim.utils", "smpl_sim.utils.transform_utils")
    saved = {n: sys.modules.get(n) for n in names}
    for n in names:
        sys.modules[n] = types.ModuleType(n)
    sys.modules[names[2]].quat_correct = _quat_correct
    try:
        yield
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


def run_reference(clip, dtype):
    """One clip through the script in ``dtype`` -> (the converted entry: field -> array, the first loop's pose_aa (F, 72) and trans (F, 3))."""
    from oracle import refload
    from scipy.spatial.transform import Rotation
    path = os.path.join(refload.REFERENCE_ROOT, "scripts", "data_process", "convert_data_mdm.py")
    ns = GI._namespace(dtype)
    ns["sRot"] = types.SimpleNamespace(from_euler=lambda seq, a, degrees=False: _Rot(Rotation.from_euler(seq, a, degrees=degrees), dtype),
                                       from_rotvec=lambda v: _Rot(Rotation.from_rotvec(v), dtype), from_quat=lambda q: _Rot(Rotation.from_quat(q), dtype))
    ns.update({"res_data": {"json_file": {"thetas": [clip["thetas"].astype(dtype)], "root_translation": [clip["root_translation"].astype(dtype)]}},
               "i": 0, "amass_data": {}, "key_name": "0"})
    exec(compile(GI._block(path, "pose_euler", "amass_data"), "<reference:convert_data_mdm:first loop>", "exec"), ns)
    first = {"euler_pose": GI._arr(ns["amass_data"]["0"]["pose_aa"], dtype), "euler_trans": GI._arr(ns["amass_data"]["0"]["trans"], dtype)}
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), _smpl_sim_stand_in():
        warnings.simplefilter("ignore")
        exec(compile(GI._block(path, "key_name_dump", "amass_full_motion_dict"), "<reference:convert_data_mdm:second loop>", "exec"), ns)
    entry = ns["amass_full_motion_dict"]["0"]
    assert entry["fps"] == 30.0 and entry["gender"] == "neutral" and entry["beta"].shape == (10,) and not np.asarray(entry["beta"]).any()
    return {k: GI._arr(entry[k], dtype) for k in FIELDS}, first


def generate(verbose=True, seed=SEED):
    clips = inputs(seed)
    out = {"num_clips": np.int64(len(clips)), "root_offset": np.asarray(ROOT_OFFSET, dtype=np.float32), "w_floor": np.float64(W_FLOOR),
           "gap_floor": np.float64(GAP_FLOOR), "margin": np.float64(MARGIN)}
    names = FIELDS + ("euler_pose", "euler_trans")
    err = {k: 0.0 for k in names}
    stages = []
    for ci, clip in enumerate(clips):
        e64, f64 = run_reference(clip, np.float64)
        e32, f32 = run_reference(clip, np.float32)
        e64.update(f64)
        e32.update(f32)
        for k in names:
            assert e64[k].shape[0] == FRAMES[ci], (ci, k)
            out[f"c{ci}_{k}"] = e64[k]
            err[k] = max(err[k], float(np.abs(e32[k].astype(np.float64) - e64[k]).max()))
        out[f"c{ci}_thetas"], out[f"c{ci}_root_translation"] = clip["thetas"], clip["root_translation"]
        res = model(clip)
        for k in names:
            want = res["trans_orig"] if k == "euler_trans" else res[k]
            assert np.abs(want - e64[k]).max() <= 1e-9, f"clip {ci} {k}: the model and the reference differ by {np.abs(want - e64[k]).max():.3e}"
        stages.append(stage_of(res))
    ok, figures = conditions(stages)
    assert all(ok.values()), f"seed {seed}: fixture conditions not met: {ok} {figures}"
    for k, v in figures.items():
        out[k] = np.float64(v)
    for k, v in err.items():
        out[f"err_{k}"] = np.float64(v)
        if verbose:
            print(f"{k:28s} max |ref32 - ref64| {v:.3e}")
    if verbose:
        print(figures)
    return out


def load():
    with np.load(PATH, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def clips_of(fx):
    """The fixture's generated clips as ``inputs`` makes them."""
    return [{"thetas": fx[f"c{i}_thetas"], "root_translation": fx[f"c{i}_root_translation"]} for i in range(int(fx["num_clips"]))]


def find_seed(start=SEED, tries=20000):
    for seed in range(start, start + tries):
        ok, figures = conditions([stage_of(model(c)) for c in inputs(seed)])
        if all(ok.values()):
            return seed, figures
    raise RuntimeError("no seed found")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.dirname(PATH))
    ap.add_argument("--find-seed", action="store_true")
    a = ap.parse_args()
    if a.find_seed:
        print(find_seed())
        return
    path = os.path.join(a.out, "mdm_ingest.npz")
    np.savez_compressed(path, **generate())
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, f"{path}: {size} bytes > {MAX_BYTES}"
    print(path, size, "bytes")


if __name__ == "__main__":
    main()
