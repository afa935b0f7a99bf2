"""The AMP observation window of HumanoidAMP (phc/env/tasks/humanoid_amp.py:91-118, 194-284, 296-314, 519-563, 622-680), held by every task
class that hands AMP observations to the discriminator: HumanoidIm (env/humanoid_im.py) and the downstream tasks (env/humanoid_tasks.py).

One object owns the (N, numAMPObsSteps, W) history -- slot 0 the current simulated frame, slots 1 .. S-1 the frames before it -- the env
options that shape the frame (numAMPObsSteps, ampRootHeightObs, key_bodies, has_dof_subset, amp_obs_v, add_amp_input_noise, the
discriminator's shape / limb rows), the per-step update (one fused launch of pulse_amp_obs: shift + current frame + the finished window
into the caller's sink), the initialisation after a reference-state reset (pulse_amp_hist_init) and the demonstration windows
(fetch_amp_obs_demo).  PULSE_AMP_FUSED=0 selects the op-by-op path (shift, frame, copy) the fused kernels are tested against.
"""
import os

import torch

from .. import ops


class Box:
    """Minimal gym.spaces.Box stand-in (gym is not installed)."""

    def __init__(self, low, high, shape):
        import numpy as np
        self.shape = tuple(shape)
        self.low = np.full(self.shape, low, dtype=np.float32)
        self.high = np.full(self.shape, high, dtype=np.float32)


class AmpWindow:
    """``env``: the env dict (robot switches merged in); ``skeleton``: synthetic.skeleton(humanoid_type); ``shape_rows`` (N, 11) /
    ``limb_rows`` (N, 10): the envs' rows behind a simulated frame, ``motion_shape_rows`` / ``motion_limb_rows``: one row per MOTION behind
    a reference frame (humanoid_amp.py:243-250, 548-555, 672); each only with its has_*_obs_disc switch."""

    def __init__(self, env, *, num_envs, device, skeleton, local_root_obs, upright, amp_obs_v, shape_rows=None, limb_rows=None,
                 motion_shape_rows=None, motion_limb_rows=None):
        dev = self.device = torch.device(device)
        sk, names = skeleton, skeleton["body_names"]
        self.num_envs = num_envs
        self.local_root_obs = bool(local_root_obs)
        self.num_steps = int(env.get("numAMPObsSteps", 10))
        self.root_height_obs = bool(env.get("ampRootHeightObs", env.get("root_height_obs", True)))
        self.key_body_ids = torch.tensor([names.index(b) for b in env.get("key_bodies", sk["key_bodies"])], dtype=torch.int32, device=dev)
        # dof_subset (humanoid.py:396-421): every joint but L_Hand / R_Hand / L_Toe / R_Toe; applied when the robot config says
        # has_dof_subset (True in robot/smpl_humanoid.yaml:6) -> 19 joints, 196 floats per frame, 1960 per window.  For SMPL the
        # subset tensor always exists, so the in-place zeroing of the toe / hand dofs (humanoid_amp.py:636-639, guarded by
        # ``dof_subset is None``) never runs on this humanoid.
        self.has_dof_subset = bool(env.get("has_dof_subset", True))
        nj = sk["num_dof"] // 3
        joint_ids = [d // 3 for d in sk["dof_subset"][::3]] if self.has_dof_subset else None
        self.zero_joints = ()
        # the frame's shape / limb rows (humanoid_amp.py:311-314, 963-966): the env's for simulated frames, the motion's for reference frames
        self.shape_rows, self.limb_rows = shape_rows, limb_rows
        self.motion_shape_rows, self.motion_limb_rows = motion_shape_rows, motion_limb_rows
        self.variant = {"upright": bool(upright), "version": int(amp_obs_v)}
        self.per_step = ops.amp_obs_width(len(joint_ids) if self.has_dof_subset else nj, self.key_body_ids.numel(), self.root_height_obs,
                                          version=int(amp_obs_v), num_shape=11 * (shape_rows is not None), num_limb=10 * (limb_rows is not None))
        self.joint_ids = torch.tensor(joint_ids, dtype=torch.int32, device=dev) if joint_ids is not None else None
        self.buf = torch.zeros(num_envs, self.num_steps, self.per_step, device=dev)
        self.fused = os.environ.get("PULSE_AMP_FUSED", "1") != "0"          # fused history update / history init kernels (0: the op-by-op path)
        self.sink = None
        self.add_input_noise = bool(env.get("add_amp_input_noise", False))  # humanoid_amp.py:135, 281-283: demo windows + 0.01 N(0, 1)
        self.last_noise = None
        self.curr = self.buf[:, 0]
        self.hist = self.buf[:, 1:]
        self.space = Box(-float("inf"), float("inf"), (self.num_obs(),))
        self._frame_kw = {"joint_ids": self.joint_ids, "local_root_obs": self.local_root_obs, "root_height_obs": self.root_height_obs}

    def num_obs(self):
        return self.num_steps * self.per_step

    def set_sink(self, rows):
        """The NEXT ``step`` writes its finished window into ``rows`` ((N, >= S W) float32, any row pitch) as well, and hands that view out."""
        self.sink = rows

    def update_hist(self):
        """humanoid_amp.py:622-631: shift the history by one slot."""
        self.hist.copy_(self.buf[:, 0:self.num_steps - 1].clone())

    def compute(self, sim, env_mask=None):
        """humanoid_amp.py:632-667 -> current frame into slot 0 of the history."""
        ops.build_amp_observations_smpl(sim.rigid_body_state, sim.dof_pos, sim.dof_vel, self.key_body_ids, zero_joints=self.zero_joints,
                                        out=self.curr, env_mask=env_mask, shape_params=self.shape_rows, limb_weights=self.limb_rows,
                                        **self._frame_kw, **self.variant)

    def step(self, sim):
        """HumanoidAMP.post_physics_step (humanoid_amp.py:194-210) -> the (N, S W) rows for extras['amp_obs']."""
        if self.fused:
            # history shift + current frame (+ the finished window straight into the caller's row, e.g. the experience-buffer slot
            # the agent registered with set_amp_obs_sink) in ONE launch
            sink = self.sink
            ops.build_amp_observations_smpl(sim.rigid_body_state, sim.dof_pos, sim.dof_vel, self.key_body_ids, zero_joints=self.zero_joints,
                                            out=self.curr, hist_steps=self.num_steps, window_out=sink, shape_params=self.shape_rows,
                                            limb_weights=self.limb_rows, **self._frame_kw, **self.variant)
            self.sink = None
            return sink[:, :self.num_obs()] if sink is not None else self.buf.view(-1, self.num_obs())
        self.update_hist()
        self.compute(sim)
        return self.buf.view(-1, self.num_obs())

    def motion_rows(self, motion_ids):
        """The shape / limb rows of reference-motion frames: motion_bodies[ids][:, :-6] / motion_limb_weights[ids] (humanoid_amp.py:243-250,
        548-555, 672), one row per queried frame."""
        return {"shape_params": self.motion_shape_rows[motion_ids] if self.motion_shape_rows is not None else None,
                "limb_weights": self.motion_limb_rows[motion_ids] if self.motion_limb_rows is not None else None}

    def init(self, sim, mask, *, lib=None, motion_ids=None, start_times=None, dt=None, bufs=None):
        """_init_amp_obs (humanoid_amp.py:519-563) for the masked envs.  Slot 0 is the current simulated frame.  With a motion library
        (``lib``) the envs were reference-state initialised, so the history slots hold the AMP frames of the motion at
        start - dt * (k + 1) (_init_amp_obs_ref, :531-563; times before the clip clamp to its first frame); without one there is no
        motion to look back into and the history repeats the first frame (_init_amp_obs_default, :526-529)."""
        self.compute(sim, env_mask=mask)
        s = self.num_steps - 1
        if lib is not None and self.fused:
            ops.amp_hist_init(lib, motion_ids, start_times, dt, mask, self.buf, self.key_body_ids, shape_params=self.motion_shape_rows,
                              limb_weights=self.motion_limb_rows, **self._frame_kw, **self.variant)
            return
        if lib is not None:
            steps = -dt * (torch.arange(0, s, device=self.device) + 1)
            times = (start_times.unsqueeze(-1) + steps).view(-1)
            ids = motion_ids.repeat_interleave(s)
            res = lib.query(ids, times, out=bufs if bufs is not None else {}, fields=("rb_records", "dof_pos", "dof_vel"))
            hist = ops.build_amp_observations_smpl(res["rb_records"], res["dof_pos"], res["dof_vel"], self.key_body_ids, zero_joints=(),
                                                   **self._frame_kw, **self.motion_rows(ids), **self.variant)
            hist = hist.view(self.num_envs, s, self.per_step)
        else:
            hist = self.curr.unsqueeze(1).expand(-1, s, -1)
        self.hist.copy_(torch.where(mask[:, None, None], hist, self.hist))

    def demo_windows(self, rb, dof_pos, dof_vel, rows, num_samples, noise_generator=None):
        """build_amp_obs_demo (humanoid_amp.py:253-284) on ``num_samples * S`` states, newest first within a window."""
        out = ops.build_amp_observations_smpl(rb, dof_pos, dof_vel, self.key_body_ids, zero_joints=(), **self._frame_kw, **rows, **self.variant)
        out = out.view(num_samples, self.num_obs())
        if self.add_input_noise:                      # build_amp_obs_demo's last statement (humanoid_amp.py:281-283)
            self.last_noise = torch.randn(out.shape, device=self.device, generator=noise_generator)
            out = out + self.last_noise * 0.01
        return out

    def fetch_demo(self, num_samples, lib, dt, generator, bufs=None):
        """fetch_amp_obs_demo (humanoid_amp.py:215-284) from a motion library: ``num_samples`` windows of reference motion.  Returns
        (windows, result buffers to hand back in next time, motion ids, start times)."""
        s = self.num_steps
        ids = lib.sample_motions(num_samples, generator=generator)
        # _sample_time (humanoid_amp.py:223-224, 376-380: sample_time_interval for smpl): start times on the 1/30 s grid, no frame blending
        t0 = lib.sample_time_interval(ids, generator=generator)
        steps = -dt * torch.arange(0, s, device=self.device)                  # build_amp_obs_demo, :256-262
        times = (t0.unsqueeze(-1) + steps).view(-1)
        bufs = bufs if bufs is not None and bufs.get("dof_pos", torch.empty(0)).shape[0] == num_samples * s else {}
        res = lib.query(ids.repeat_interleave(s), times, out=bufs, with_records=True)
        out = self.demo_windows(res["rb_records"], res["dof_pos"], res["dof_vel"], self.motion_rows(ids.repeat_interleave(s)), num_samples,
                                noise_generator=generator)
        return out, res, ids, t0
