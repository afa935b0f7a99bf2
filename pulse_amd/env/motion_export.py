"""The way back out of the motion library: a recorded rollout -> motion clips and SMPL pose sequences, on the device.

The reference records ``dof_pos`` / ``root_states`` / ``progress`` every step with a copy to the host (Humanoid._record_states,
phc/env/tasks/humanoid.py:430-437), cuts the recording into episodes at the jumps of ``progress`` and dumps one dict per episode
(_write_states_to_file, :439-491); HumanoidIm.render turns the simulator's body rotations back into SMPL ``pose_aa`` / ``trans`` frame by frame
with scipy and poselib (phc/env/tasks/humanoid_im.py:217-257), the inverse of scripts/data_process/convert_amass_isaac.py:85-137.  Here:

  * ``MotionRecorder`` keeps the recording in preallocated device buffers (no host sync per step);
  * ``segment_recording`` applies the reference's episode rule to the recorded ``progress`` on the device;
  * ``export_motion`` converts every frame of every segment in ONE launch of ``pulse_motion_export`` (csrc/motion_export.hip, include/pulse_hip.h
    section 2b'.2) and hands back CPU numpy arrays in the layout ``MotionLib.motion_data()`` / ``from_motion_data`` speak (form "motion") or in the
    layout of the reference's dump (form "states").  Writing a file stays with the caller: ``joblib.dump(export, path)`` is the reference's last line.
"""
import warnings

import torch

SENTINEL = -10                      # humanoid.py:445
FORMS = ("motion", "states")
GENDERS = ("neutral", "male", "female")


class MotionExport(dict):
    """key -> clip dict, in the reference's order; ``dropped``: [(key, frames)] of the segments shorter than ``min_frames``; ``segments``: the
    kept segments' {"keys", "env", "t0", "frames"} (where every clip sits in the recording)."""
    dropped = ()
    segments = None

    @property
    def dropped_frames(self):
        return sum(f for _, f in self.dropped)

    def __reduce__(self):
        # written to a file (joblib.dump, pickle) it is the plain dict of clips, loadable where this package is not installed (the reference's loader)
        return (dict, (dict(self),))


def segment_recording(progress):
    """The reference's episode rule (humanoid.py:444-470) on a (T, N) int64 recording of ``progress_buf`` ON THE DEVICE: the sentinel -10 is
    appended, and a segment ends after step t where |progress[t] - progress[t + 1]| > 1.  -> {"env", "t0", "frames": (M) int64 CPU tensors,
    "keys": [f"{env}_{k}"]} in the reference's order (env-major, then time); every env's segments partition [0, T).  The reference's quirk is
    kept: a reset that moves ``progress`` by 1 or less (an episode that ends at its first step) does not split.  The last step always ends a
    segment, as it does in the reference for any progress >= 0.  Torch ops and one read-back of the boundary list; the per-frame work is the kernel's."""
    if not isinstance(progress, torch.Tensor) or progress.dim() != 2 or progress.dtype != torch.int64:
        raise TypeError("segment_recording: progress (T, N) int64 tensor expected")
    steps, envs = progress.shape
    if steps == 0 or envs == 0:
        empty = torch.zeros(0, dtype=torch.int64)
        return {"env": empty, "t0": empty.clone(), "frames": empty.clone(), "keys": []}
    ext = torch.cat([progress, torch.full((1, envs), SENTINEL, dtype=torch.int64, device=progress.device)])
    split = (ext[:-1] - ext[1:]).abs() > 1
    split[-1] = True
    ends = split.t().nonzero()                                  # (M, 2) rows (env, t), env-major then time
    env, end = ends[:, 0], ends[:, 1] + 1
    first = torch.ones_like(env, dtype=torch.bool)
    first[1:] = env[1:] != env[:-1]
    t0 = torch.where(first, torch.zeros_like(end), end.roll(1))
    idx = torch.arange(env.numel(), device=env.device)
    k = idx - torch.where(first, idx, torch.zeros_like(idx)).cummax(0).values
    host = torch.stack([env, t0, end - t0, k]).cpu()            # the one read-back
    return {"env": host[0].contiguous(), "t0": host[1].contiguous(), "frames": host[2].contiguous(),
            "keys": [f"{e}_{i}" for e, i in zip(host[0].tolist(), host[3].tolist())]}


def export_motion(rb, progress, skeleton_trees, *, dof_pos=None, upright_start=True, root_offset=None, fps=None, dt=None, form="motion",
                  min_frames=1, betas=None):
    """A recording -> {f"{env}_{k}": clip} (``MotionExport``, CPU numpy arrays), one clip per episode segment of ``segment_recording(progress)``.

    ``rb`` (T, N, J, 13) rigid-body states and ``progress`` (T, N) int64 on the device, read in place (any view with unit inner stride);
    ``dof_pos`` (T, N, 3 (J - 1)) optional; ``skeleton_trees`` as ``MotionLib.from_motion_data`` takes them.

      * form "motion": the converted-data layout ``MotionLib.motion_data()`` speaks -- pose_quat_global, pose_quat, trans_orig, root_trans_offset,
        beta, gender, pose_aa, fps.  ``MotionLib.from_motion_data`` takes the dict as it is; ``from_smpl_data`` takes pose_aa / trans_orig as
        poses / trans.  With ``upright_start`` pose_quat / pose_aa are render()'s (humanoid_im.py:234-238); without, pose_aa is
        [quat_to_exp_map(root_rot), dof_pos] reordered (:240-257) and pose_quat [root quat, exp_map_to_quat(dof_pos)] (needs ``dof_pos``);
      * form "states": the keys of _write_states_to_file -- body_quat, trans, root_states_seg, dof_pos, fps, betas (needs ``dof_pos``).  The
        ``skeleton_tree`` dict of the dump is the caller's, as it is in ``from_motion_data``;
      * ``fps`` defaults to round(1 / ``dt``), the control rate: ``dt`` is the control step in seconds (``MotionRecorder.export`` passes the task's),
        needed only where ``fps`` is not given.  The reference writes the literal 60 whatever the control rate (humanoid.py:452):
        ``fps=60`` reproduces its file;
      * ``root_offset``: three floats subtracted from the root position for trans_orig (default: local_translation[0] of skeleton slot 0, as in
        ``from_smpl_data``);
      * segments shorter than ``min_frames`` are dropped and counted in a warning that names them (``MotionLib.from_motion_data`` needs 2);
      * ``betas`` (N, 17) = the task's humanoid_shapes [gender, 10 betas, 6 unused]: "motion" takes gender and beta from it (beta is always 16
        long, as the conversion script writes it: the 10 betas, then zeros; default: neutral, zeros), "states" the whole row.
    Pickled (``joblib.dump``), the result is a plain dict of the clips: ``dropped`` and ``segments`` stay with the object in memory.
    One export is one ``pulse_motion_export`` launch.  Only the 24-body SMPL humanoid is built: SMPL-X / SMPL-H raise by name, as ingest does."""
    import numpy as np
    from .. import kernels, synthetic
    from .motion_lib import _parse_skeleton_trees
    if form not in FORMS:
        raise ValueError(f"export_motion: form {form!r}: one of {FORMS}")
    parents, lt = _parse_skeleton_trees(skeleton_trees)
    joint_map = synthetic.smpl_joint_map()
    if len(parents) != len(joint_map):
        raise NotImplementedError(f"export_motion: the skeleton trees have {len(parents)} bodies: only the 24-body SMPL humanoid is built "
                                  "(SMPL-X / SMPL-H export: mujoco_2_smpl over SMPLH_BONE_ORDER_NAMES, humanoid_im.py:165-166)")
    if not isinstance(rb, torch.Tensor) or not rb.is_cuda:
        raise TypeError("export_motion: rb must be a CUDA tensor (pulse_amd has no CPU path)")
    j = len(parents)
    if rb.dim() != 4 or tuple(rb.shape[2:]) != (j, 13) or tuple(progress.shape) != tuple(rb.shape[:2]):
        raise ValueError(f"export_motion: rb (T, N, {j}, 13) and progress (T, N) expected, got {tuple(rb.shape)} and {tuple(progress.shape)}")
    if form == "states" and dof_pos is None:
        raise ValueError("export_motion: form 'states' needs dof_pos (body_quat = [root quat, exp_map_to_quat(dof_pos)])")
    if form == "motion" and not upright_start and dof_pos is None:
        raise ValueError("export_motion: without upright_start pose_aa is [quat_to_exp_map(root_rot), dof_pos]: dof_pos is needed")
    if fps is None:
        if dt is None:
            raise ValueError("export_motion: fps or dt (the control step; fps = round(1 / dt)) is needed")
        fps = int(round(1.0 / float(dt)))
    seg = segment_recording(progress.to(rb.device))
    keep = seg["frames"] >= int(min_frames)
    out = MotionExport()
    out.dropped = [(k, int(f)) for k, f, ok in zip(seg["keys"], seg["frames"].tolist(), keep.tolist()) if not ok]
    if out.dropped:
        warnings.warn(f"export_motion: dropped {len(out.dropped)} segment(s) shorter than {int(min_frames)} frame(s) "
                      f"({out.dropped_frames} frames): {', '.join(k for k, _ in out.dropped)}")
    keys = [k for k, ok in zip(seg["keys"], keep.tolist()) if ok]
    seg_env, seg_t0, frames = (seg[k][keep].contiguous() for k in ("env", "t0", "frames"))
    total, dev = int(frames.sum()), rb.device
    out.segments = {"keys": keys, "env": seg_env, "t0": seg_t0, "frames": frames}
    if not keys:
        return out
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
    if form == "motion":
        dev_out = {"out_pose_quat": new(total, j, 4), "out_pose_aa": new(total, 3 * j), "out_trans_orig": new(total, 3)}
    else:
        dev_out = {"out_body_quat": new(total, j, 4), "out_dof_pos": new(total, 3 * (j - 1))}
    off = lt[0, 0].tolist() if root_offset is None else [float(v) for v in root_offset]
    rot, trans = new(total, j, 4), new(total, 3)
    kernels.motion_export(rot, trans, rb=rb, dof_pos=dof_pos, seg_env=seg_env, seg_t0=seg_t0, seg_frames=frames, parents=parents, joint_map=joint_map,
                          upright_start=upright_start, root_offset=off, **dev_out)
    host = {"rot": rot.cpu().numpy(), "trans": trans.cpu().numpy(), **{k[4:]: v.cpu().numpy() for k, v in dev_out.items()}}
    if form == "states":
        # root_states_seg: the root's whole 13-float row (humanoid.py:475), a plain gather of the recording
        tt = torch.cat([torch.arange(t, t + f) for t, f in zip(seg_t0.tolist(), frames.tolist())]).to(dev)
        ee = torch.repeat_interleave(seg_env, frames).to(dev)
        host["root_states"] = rb[tt, ee, 0].cpu().numpy()
    shapes = None if betas is None else torch.as_tensor(betas).detach().cpu().numpy()
    def beta_of(e):                                              # 16 values, as the conversion script writes them; the humanoid's 10 betas first
        beta = np.zeros(16)
        if shapes is not None:
            beta[:10] = shapes[e, 1:11]
        return beta

    at = 0
    for key, e, f in zip(keys, seg_env.tolist(), frames.tolist()):
        s = slice(at, at + f)
        at += f
        if form == "motion":
            gender = GENDERS[int(shapes[e, 0])] if shapes is not None and 0 <= int(shapes[e, 0]) < 3 else "neutral"
            out[key] = {"pose_quat_global": host["rot"][s].copy(), "pose_quat": host["pose_quat"][s].copy(), "trans_orig": host["trans_orig"][s].copy(),
                        "root_trans_offset": host["trans"][s].copy(), "beta": beta_of(e),
                        "gender": gender, "pose_aa": host["pose_aa"][s].copy(), "fps": fps}
        else:
            out[key] = {"body_quat": host["body_quat"][s].copy(), "trans": host["trans"][s].copy(), "root_states_seg": host["root_states"][s].copy(),
                        "dof_pos": host["dof_pos"][s].copy(), "fps": fps, "betas": np.zeros(17, dtype=np.float32) if shapes is None else shapes[e].copy()}
    return out


class MotionRecorder:
    """The reference's recorder surface (_record_states / _clear_recorded_states / _write_states_to_file) on the device: ``record()`` after a step
    copies the task's rigid_body_state, dof_pos and progress_buf into preallocated buffers of ``capacity`` steps -- three device copies, no
    host sync; ``clear()``; ``export(...)`` -> ``export_motion`` of what was recorded.  Works for HumanoidIm and the downstream tasks: both carry
    ``sim`` (rigid_body_state, dof_pos), ``progress_buf``, ``dt`` and ``_has_upright_start``."""

    def __init__(self, task, capacity):
        sim = task.sim
        if int(capacity) < 1:
            raise ValueError(f"MotionRecorder: capacity {capacity} < 1")
        self.task, self.capacity, self.steps = task, int(capacity), 0
        dev = sim.rigid_body_state.device
        self.rb = torch.empty((self.capacity,) + tuple(sim.rigid_body_state.shape), dtype=torch.float32, device=dev)
        self.dof_pos = torch.empty((self.capacity,) + tuple(sim.dof_pos.shape), dtype=torch.float32, device=dev)
        self.progress = torch.empty((self.capacity,) + tuple(task.progress_buf.shape), dtype=torch.int64, device=dev)

    def record(self):
        if self.steps >= self.capacity:
            raise RuntimeError(f"MotionRecorder: the {self.capacity} steps of capacity are used up (clear() or export first)")
        t, task = self.steps, self.task
        self.rb[t].copy_(task.sim.rigid_body_state)
        self.dof_pos[t].copy_(task.sim.dof_pos)
        self.progress[t].copy_(task.progress_buf)
        self.steps = t + 1

    def clear(self):
        self.steps = 0

    def skeleton_trees(self):
        """The trees the task's motion library was last loaded with, or the humanoid's parents with no root offset."""
        from .. import synthetic
        last = getattr(getattr(self.task, "_motion_lib", None), "_last_load", None)
        if last and last.get("skeleton_trees") is not None:
            return last["skeleton_trees"]
        parents = synthetic.skeleton(getattr(self.task, "humanoid_type", "smpl"))["parents"]
        return list(parents), torch.zeros(1, len(parents), 3)

    def export(self, skeleton_trees=None, **kw):
        if self.steps == 0:
            raise ValueError("MotionRecorder.export: nothing recorded")
        task, t = self.task, self.steps
        kw.setdefault("upright_start", bool(getattr(task, "_has_upright_start", True)))
        kw.setdefault("betas", getattr(task, "humanoid_shapes", None))
        if kw.get("fps") is None:
            kw.setdefault("dt", task.dt)
        return export_motion(self.rb[:t], self.progress[:t], skeleton_trees if skeleton_trees is not None else self.skeleton_trees(),
                             dof_pos=self.dof_pos[:t], **kw)
