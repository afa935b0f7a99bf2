"""Generate tests/golden/keypoint_stream.npz: what the reference computes from streamed keypoints, for pulse_keypoint_push to be held to.

    python tools/gen_golden_keypoint_stream.py [--out DIR] [--find-seed]

Needs the reference tree and scipy.  Nothing of the reference's text is kept here: the body of HumanoidImMCPDemo._compute_task_obs_demo
(phc/env/tasks/humanoid_im_mcp_demo.py) is extracted by name with oracle.refload._extract and executed against a stub ``self``, with
  * a local stand-in object under the name ``requests`` that hands back canned frames (nothing here imports the real one, opens a socket or
    resolves a host); it is in the namespace before the body is compiled and executed;
  * ``filters`` = scipy.ndimage;
  * ``SkeletonMotion._compute_velocity``: the reference's own (poselib skeleton3d.py), extracted the same way; its result is also kept, because
    the body holds the velocity in a local only;
  * ``compute_imitation_observations_v7`` from refload.env_functions();
  * ``smpl_2_mujoco`` read from the module's own assignment (and checked against synthetic.smpl_joint_map());
  * ``Tensor.cuda`` handing back the tensor for the call.
The constructor's constants (to_isaac_mat, mean_limb_lengths, s_dt, close_distance = 0.5, zeroed prev_ref_body_pos, the deques) are set on the
stub as lines 50-66 set them.

Streams, 5 envs each, rigid-body frames from RecordedRollout(5, 37, SEED):
  A   37 frames at history 30: L = 1 .. 30, then seven wrapped pushes;
  B    7 frames at history 4.
The recorded rigid-body frames are independent draws per step (root xy ~ N(0, 1)), and the filtered reference is a weighted mean of up to 30
frames, so no keypoint stream stays within 0.5 m of such a root at every step.  The three masking regimes are therefore covered per STEP, not per
env: envs 0 .. 2 take turns (step t: env t mod 3) at having their FILTERED root land on the simulated root -- their keypoint roots are the
minimum-norm solution of those linear conditions, a few metres large -- env 3 stays a metre or two off and env 4 stays 9 m off.  The tool asserts,
with the fp64 model, that every step has an env within close_distance, one between it and far_distance and one beyond, and that no distance is
within 1e-3 of a threshold.

Stored per step: the inputs, ``pos`` / ``vel`` / ``obs`` of the reference body (float32, as it computes them), ``pos64`` / ``vel64`` of
tests/keypoint_stream_model.py in float64, and  err_pos / err_vel = max |model(float32 staging) - model(float64)|  over both streams: the error of
an fp32 evaluation of the reference's own statements, the only thing the GPU test's tolerance is made of.
"""
import argparse
import ast
import collections
import contextlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import keypoint_stream_model as KM  # noqa: E402
from pulse_amd import kernels  # noqa: E402
from pulse_amd import synthetic as syn  # noqa: E402

SEED = 4101                                          # the first seed from 4100 whose streams meet regimes() (--find-seed)
MAX_BYTES = 1 << 20
PATH = os.path.join(ROOT, "tests", "golden", "keypoint_stream.npz")
N, J = 5, 24
STREAMS = {"A": (37, 30), "B": (7, 4)}               # name -> (frames, history)
CLOSE, FAR, MARGIN = 0.5, 3.0, 1e-3
JITTER = 0.01


# ---------------------------------------------------------------------------------------------------------------- the inputs
def rollout_rb(seed=SEED):
    from pulse_amd.env.sim import RecordedRollout
    return RecordedRollout(N, STREAMS["A"][0], seed=seed).data["rb"].numpy().copy()           # (37, 5, 24, 13) float32


def _filter_matrix(frames, history, table):
    """(T, T): row t holds the weights with which the filtered sample of step t combines the pushed samples."""
    taps = kernels.keypoint_taps(history=history)
    a = np.zeros((frames, frames))
    for t in range(frames):
        length = min(t + 1, history)
        a[t, t - length + 1:t + 1] = taps[table, length - 1, :length]
    return a


def keypoints(rb, frames, history, seed):
    """(T, 5, 24, 3) float32 keypoints in SMPL joint order, y-up frame (module docstring)."""
    rng = np.random.default_rng(seed)
    frame = kernels.keypoint_frame("y_up")
    sim_root = rb[:frames, :, 0, 0:3].astype(np.float64)                                    # (T, N, 3)
    want = sim_root @ frame                                                                 # frame^T x: the simulated root in the keypoints' frame
    root = np.zeros((frames, N, 3))
    for e in range(3):                                                                      # the envs that take turns at the near regime
        duty = np.arange(frames) % 3 == e
        for c in range(3):
            a = _filter_matrix(frames, history, 0 if c == 2 else 1)[duty]
            root[:, e, c] = np.linalg.pinv(a) @ want[duty, e, c]
    off = {3: np.array([1.4, 0.0, 0.3]), 4: np.array([9.0, 0.0, -2.0])}
    for e, o in off.items():
        root[:, e] = want[:, e].mean(0) + o + 0.02 * np.cumsum(rng.standard_normal((frames, 3)), axis=0)
    # a fixed body shape per env: every body hangs on its parent, limbs 1 .. 5 at the mean lengths times the env's size
    jm, parents = syn.smpl_joint_map(), syn.SMPL_PARENTS
    size = np.array([0.8, 0.95, 1.0, 1.1, 1.3])
    shape = np.zeros((N, J, 3))
    for b in range(1, J):
        d = rng.standard_normal((N, 3))
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        length = kernels.KEYPOINT_MEAN_LIMB_LENGTHS[b - 1] if b <= 5 else 0.1 + 0.25 * rng.random()
        shape[:, b] = shape[:, parents[b]] + d * length * size[:, None]
    body = root[:, :, None, :] + shape[None] + JITTER * rng.standard_normal((frames, N, J, 3))
    body[:, :, 0] = root
    j3d = np.zeros_like(body)
    j3d[:, :, jm] = body                                                                    # body b sits at SMPL joint jm[b]
    return j3d.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the reference
@contextlib.contextmanager
def _cuda_is_here():
    keep = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.Tensor.cuda = keep


def _module_list(path, name):
    with open(path) as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError(f"{name} not found in {path}")


def run_reference(j3d, rb, history, far_distance=FAR):
    """The reference body, step by step -> pos, vel (T, N, 24, 3), obs (T, N, 216), float32 as it computes them."""
    import scipy.ndimage
    from scipy.spatial.transform import Rotation as sRot
    from oracle import refload
    path = os.path.join(refload.REFERENCE_ROOT, "phc", "env", "tasks", "humanoid_im_mcp_demo.py")
    src = refload._extract(path, ["_compute_task_obs_demo"], methods_of="HumanoidImMCPDemo")["_compute_task_obs_demo"]
    smpl_2_mujoco = _module_list(path, "smpl_2_mujoco")
    assert smpl_2_mujoco == syn.smpl_joint_map()
    pl = os.path.join(refload.REFERENCE_ROOT, "poselib", "poselib", "skeleton", "skeleton3d.py")
    vns = {"np": np, "torch": torch, "filters": scipy.ndimage}
    exec(compile(refload._extract(pl, ["_compute_velocity"], methods_of="SkeletonMotion")["_compute_velocity"], "<reference:_compute_velocity>", "exec"), vns)
    kept = {}

    def compute_velocity(p, time_delta, guassian_filter=True):
        kept["vel"] = vns["_compute_velocity"](p, time_delta=time_delta, guassian_filter=guassian_filter)
        return kept["vel"]

    canned = {}

    class _Response:
        def json(self):
            return {"j3d": canned["frame"]}

    ns = {"torch": torch, "np": np, "requests": types.SimpleNamespace(get=lambda url: _Response()), "filters": scipy.ndimage,
          "SkeletonMotion": types.SimpleNamespace(_compute_velocity=compute_velocity), "SERVER": "0.0.0.0", "smpl_2_mujoco": smpl_2_mujoco,
          "humanoid_im": types.SimpleNamespace(compute_imitation_observations_v7=refload.env_functions()["compute_imitation_observations_v7"])}
    exec(compile(src, "<reference:HumanoidImMCPDemo._compute_task_obs_demo>", "exec"), ns)
    n = j3d.shape[1]
    me = types.SimpleNamespace(
        num_envs=n, device="cpu", obs_v=7, _track_bodies_id=torch.arange(J), _has_upright_start=True, zero_out_far=True, close_distance=CLOSE,
        far_distance=far_distance, skeleton_trees=[types.SimpleNamespace(parent_indices=torch.tensor(syn.SMPL_PARENTS))],
        mean_limb_lengths=np.array(kernels.KEYPOINT_MEAN_LIMB_LENGTHS, dtype=np.float32)[None, :],
        to_isaac_mat=torch.from_numpy(sRot.from_euler("xyz", np.array([-np.pi / 2, 0, 0]), degrees=False).as_matrix()).float(),
        prev_ref_body_pos=torch.zeros(n, J, 3), root_pos_acc=collections.deque(maxlen=history), body_pos_acc=collections.deque(maxlen=history))
    assert np.array_equal(me.to_isaac_mat.numpy(), kernels.keypoint_frame("y_up").astype(np.float32))
    pos, vel, obs = [], [], []
    for t in range(j3d.shape[0]):
        canned["frame"] = j3d[t].astype(np.float64)
        frame = torch.from_numpy(rb[t])
        me._rigid_body_pos, me._rigid_body_rot = frame[..., 0:3].clone(), frame[..., 3:7].clone()
        me._rigid_body_vel, me._rigid_body_ang_vel = frame[..., 7:10].clone(), frame[..., 10:13].clone()
        with _cuda_is_here(), np.errstate(invalid="raise", divide="raise"):
            o = ns["_compute_task_obs_demo"](me)
        assert np.array_equal(me.ref_body_pos_subset.numpy(), j3d[t][:, smpl_2_mujoco].astype(np.float64))        # the markers: the reordered input
        pos.append(me.prev_ref_body_pos.numpy().copy())
        vel.append(kept["vel"][:, 0].numpy().copy())
        obs.append(o.numpy().copy())
    out = np.stack(pos), np.stack(vel), np.stack(obs)
    assert all(v.dtype == np.float32 for v in out)
    return out


def regimes(pos64, rb):
    """Distances (T, N) of the filtered reference root from the simulated root, and the tool's conditions on them."""
    d = np.linalg.norm(rb[:pos64.shape[0], :, 0, 0:3].astype(np.float64) - pos64[:, :, 0], axis=-1)
    assert (np.abs(d - CLOSE) > MARGIN).all() and (np.abs(d - FAR) > MARGIN).all(), "a distance sits within 1e-3 of a threshold"
    near, far = d < CLOSE, d > FAR
    mid = ~near & ~far
    assert near.any(1).all() and mid.any(1).all() and far.any(1).all(), "a step misses a masking regime"
    return d


def generate(verbose=True, seed=SEED):
    rb = rollout_rb(seed)
    out = {"rb": rb, "close_distance": np.float64(CLOSE), "far_distance": np.float64(FAR), "seed": np.int64(seed),
           "mean_limb_lengths": np.array(kernels.KEYPOINT_MEAN_LIMB_LENGTHS, dtype=np.float32), "frame": kernels.keypoint_frame("y_up").astype(np.float32)}
    err_pos = err_vel = 0.0
    for name, (frames, history) in STREAMS.items():
        j3d = keypoints(rb, frames, history, seed + ord(name))
        pos64, vel64 = KM.run(j3d, history, np.float64)
        pos32, vel32 = KM.run(j3d, history, np.float32)
        assert pos32.dtype == np.float32 and vel32.dtype == np.float32
        d = regimes(pos64, rb)
        pos, vel, obs = run_reference(j3d, rb, history)
        out.update({f"j3d_{name}": j3d, f"pos_{name}": pos, f"vel_{name}": vel, f"obs_{name}": obs, f"pos64_{name}": pos64, f"vel64_{name}": vel64,
                    f"dist_{name}": d, f"history_{name}": np.int64(history)})
        err_pos = max(err_pos, float(np.abs(pos32.astype(np.float64) - pos64).max()))
        err_vel = max(err_vel, float(np.abs(vel32.astype(np.float64) - vel64).max()))
        if verbose:
            print(f"stream {name}: {frames} frames, history {history}; max |pos| {np.abs(pos64).max():.2f} m, max |keypoint| {np.abs(j3d).max():.2f} m; "
                  f"near / mid / far envs per step: {(d < CLOSE).sum(1).min()}+ / {((d > CLOSE) & (d < FAR)).sum(1).min()}+ / {(d > FAR).sum(1).min()}+")
    out["err_pos"], out["err_vel"] = np.float64(err_pos), np.float64(err_vel)
    if verbose:
        print(f"err_pos {err_pos:.3e}  err_vel {err_vel:.3e}  (max |model32 - model64| over both streams)")
    return out


def load():
    with np.load(PATH, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def find_seed(start=4100, tries=100):
    for seed in range(start, start + tries):
        rb = rollout_rb(seed)
        try:
            for name, (frames, history) in STREAMS.items():
                regimes(KM.run(keypoints(rb, frames, history, seed + ord(name)), history, np.float64)[0], rb)
        except AssertionError:
            continue
        return seed
    raise RuntimeError("no seed found")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.dirname(PATH))
    ap.add_argument("--find-seed", action="store_true")
    a = ap.parse_args()
    if a.find_seed:
        print(find_seed())
        return
    path = os.path.join(a.out, "keypoint_stream.npz")
    np.savez_compressed(path, **generate())
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, f"{path}: {size} bytes > {MAX_BYTES}"
    print(path, size, "bytes")


if __name__ == "__main__":
    main()
