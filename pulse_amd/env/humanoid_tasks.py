"""Downstream tasks on MI355X: HumanoidSpeed / HumanoidReach / HumanoidStrike and their latent-action (Z) forms.

Mirrors (the tasks a frozen PULSE decoder is trained on, README "pulse_z_task" commands):
  HumanoidAMPTask        phc/env/tasks/humanoid_amp_task.py   observation = [self obs | task obs], _update_task / _reset_task hooks
  HumanoidSpeed(Z)       phc/env/tasks/humanoid_speed.py:22-343
  HumanoidReach(Z)       phc/env/tasks/humanoid_reach.py:19-250
  HumanoidStrike(Z)      phc/env/tasks/humanoid_strike.py:21-380
  Humanoid._compute_reset / compute_humanoid_reset   phc/env/tasks/humanoid.py:1066-1075, 1572-1608
Per control step the env side is TWO launches: the self observation of the fused env-step kernel (pulse_im_step, SELF_OBS only)
and pulse_task_step (task observation at its column offset of the same GEMM-ready row, reward, reset / terminate flags).
The target bookkeeping (_update_task / _reset_task: new target speed / position every tarChangeSteps) is sync-free masked
tensor code -- the reference reads ``nonzero()`` back every step.

The HumanoidAMP layer every one of these classes inherits in the reference (HumanoidAMPTask -> HumanoidAMP, humanoid_amp_task.py:33,
humanoid_amp.py:72) is opt-in through ``enable_amp_obs`` (default False: nothing below runs, same launches, draws and buffers) and needs
a MotionLib (``motion_lib=``):
  reset from motion      _reset_ref_state_init with the task's _sample_ref_state (humanoid_amp.py:447-488; humanoid_speed.py:251-270,
                         humanoid_reach.py:46-49, humanoid_strike.py:147-150, humanoid_pedestrian_terrain.py:488-589): a new clip and start
                         time per reset, ONE launch of pulse_task_ref_state_init (csrc/task_reset.hip) that writes the simulator's state
                         tensors, the start time, the motion id and clears the episode words
  AMP window             numAMPObsSteps frames, initialised from that clip (pulse_amp_hist_init), advanced by one fused launch per step
  AMP observation        extras["amp_obs"], set_amp_obs_sink, _amp_obs_space (AMPAgent then trains its discriminator beside the policy)
  demonstration windows  fetch_amp_obs_demo
The window itself is env/amp_window.py, shared with HumanoidIm.  The state the reset writes is the consistent one: the root record is
the reference's root state, every other body is carried rigidly by the same root transform (include/pulse_hip.h).
Out of scope: stateInit Default / Hybrid, shape rows for the discriminator, fix_trans_height, a real walkable map
(Terrain.sample_valid_locations: the terrain task draws its new location uniformly from the interior of the height field).

Physics is out of scope (Isaac Gym): ``sim`` is any object with the tensor surface of pulse_amd/env/sim.py (rigid_body_state,
dof_force, dof_vel, contact_forces and, for strike, target_states / target_contact_forces).
"""
import math

import torch

from .. import ops
from .. import synthetic as syn
from .._lib import PULSE_IM_SELF_OBS, TASK_OBS, TASK_RESET, TASK_REWARD
from . import env_keys, robot_keys
from .actuation import Actuation
from .amp_window import AmpWindow
from .humanoid_z import HumanoidZ


class HumanoidTask:
    TASK = None
    REF_STATE_TRANSFORM = "none"                    # the class's _sample_ref_state override, as a transform of ops.task_ref_state_init

    def __init__(self, cfg, sim, device="cuda:0", motion_lib=None):
        from .humanoid_im import check_humanoid_options
        check_humanoid_options(cfg, type(self).__name__)     # cfg.robot.humanoid_type: the downstream tasks are built for SMPL (raises by name otherwise)
        env = cfg.get("env", cfg)
        env_keys.audit(env, type(self).__name__)             # every key is honoured, inert by contract, or raises by name
        robot_keys.audit(cfg.get("robot", None), type(self).__name__, syn.SMPL_BODY_NAMES, unread=robot_keys.TASK_UNREAD)   # the same for cfg.robot
        if isinstance(cfg.get("robot", None), dict) and "has_upright_start" in cfg["robot"]:    # humanoid.py:355 reads it from cfg.robot; the env dict's wins
            env = dict({"has_upright_start": cfg["robot"]["has_upright_start"]}, **env)
        self.cfg, self.sim = cfg, sim
        self.device = torch.device(device)
        self.num_envs, self.num_bodies = sim.num_envs, syn.NUM_BODIES
        self.dt = int(env.get("controlFrequencyInv", 2)) / 60.0             # base_task.py:92-93
        self._local_root_obs = bool(env.get("local_root_obs", True))
        self._root_height_obs = bool(env.get("root_height_obs", True))
        self._has_upright_start = bool(env.get("has_upright_start", True))
        self._enable_task_obs = bool(env.get("enableTaskObs", True))
        self._enable_early_termination = bool(env.get("enableEarlyTermination", True))
        self.max_episode_length = int(env.get("episode_length", 300))
        self.power_reward = bool(env.get("power_reward", False))
        self.power_coefficient = float(env.get("power_coefficient", 0.0005))
        self._dof_size = syn.NUM_DOF
        # the actuation stage (humanoid.py:1037-1111, 1222-1247): the table from the simulator's joint limits, the freeze switches of cfg.robot
        self._actuation = Actuation(syn.skeleton("smpl"), cfg.get("robot", None), sim, self.device, upright=self._has_upright_start)
        self._pd_action_offset, self._pd_action_scale = self._actuation.offset, self._actuation.scale
        # power_usage_reward (humanoid_speed.py:43-53, 225-238; humanoid_strike.py:37-40, 186-198): a penalty on the difference between the
        # accumulated |torque x velocity| of the left and the right joints.  Only those two task classes read the key.
        self.power_usage_reward = bool(env.get("power_usage_reward", False)) and self.TASK in ("speed", "strike")
        self.power_usage_coefficient = float(env.get("power_usage_coefficient", 0.0025))
        if self.power_usage_reward:
            dof_names = syn.SMPL_BODY_NAMES[1:]                                        # humanoid.py: _dof_names = body names without the root
            lower = ("Hip", "Knee", "Ankle", "Toe")                                    # the strike task balances the legs only (left_lower_indexes, humanoid.py:425-426)
            pick = lambda side: [i for i, nm in enumerate(dof_names) if nm.startswith(side) and (self.TASK == "speed" or nm[2:] in lower)]
            self._left_idx = torch.tensor(pick("L"), dtype=torch.int64, device=self.device)
            self._right_idx = torch.tensor(pick("R"), dtype=torch.int64, device=self.device)
            self.power_acc = torch.zeros(self.num_envs, 2, device=self.device)
        lib = ops._lib.load()
        self._self_obs_size = lib.pulse_self_obs_width(self.num_bodies, int(self._root_height_obs))
        self._task_obs_size = self._task_obs_width(env) if self._enable_task_obs else 0
        self.num_obs = self._self_obs_size + self._task_obs_size
        self.num_actions = self._dof_size
        self.obs_pitch = (self.num_obs + 31) // 32 * 32
        n, dev = self.num_envs, self.device
        self._obs_store = torch.zeros(n, self.obs_pitch, device=dev)
        self.obs_buf = self._obs_store[:, :self.num_obs]
        self.rew_buf = torch.zeros(n, device=dev)
        self.reward_raw = torch.zeros(n, self._reward_raw_width(), device=dev)
        self.reset_buf = torch.ones(n, dtype=torch.int64, device=dev)
        self.progress_buf = torch.zeros(n, dtype=torch.int64, device=dev)
        self._terminate_buf = torch.zeros(n, dtype=torch.int64, device=dev)
        self._prev_root_pos = torch.zeros(n, 3, device=dev)
        # humanoid.py:237 reads contact_bodies (env_pulse_amp.yaml:63); contactBodies is the legacy spelling (phc_*_iccv.yaml)
        contact = env.get("contact_bodies", env.get("contactBodies", ["R_Ankle", "L_Ankle", "R_Toe", "L_Toe"]))
        self._contact_body_ids = torch.tensor([syn.SMPL_BODY_NAMES.index(b) for b in contact], dtype=torch.int32, device=dev)
        self._termination_heights = torch.full((self.num_bodies,), float(env.get("terminationHeight", 0.15)), device=dev)
        self._task_gen = torch.Generator(device=dev)
        self._task_gen.manual_seed(int(env.get("task_seed", 77)))
        self.extras = {}
        self.humanoid_type, self.has_task, self.viewer = "smpl", True, None
        self.temp_running_mean = bool(env.get("temp_running_mean", True))
        self.save_kin_info = self.only_kin_loss = False
        self.z_type = env.get("z_type", None)
        self._enable_amp_obs = bool(env.get("enable_amp_obs", False))
        self._motion_lib = motion_lib
        if self._enable_amp_obs:
            self._init_amp(cfg, env)

    # ---- the HumanoidAMP layer (humanoid_amp.py:72-135, 194-284, 447-563)
    def _init_amp(self, cfg, env):
        from .humanoid_im import check_amp_options
        name, lib, dev, n = type(self).__name__, self._motion_lib, self.device, self.num_envs
        if isinstance(cfg.get("robot", None), dict):                            # robot/*.yaml switches (humanoid.py:266-280 reads cfg.robot)
            env = dict({k: v for k, v in cfg["robot"].items() if k in ("has_dof_subset", "has_shape_obs_disc", "has_weight_obs_disc")}, **env)
        if lib is None:
            raise ValueError(f"{name}: enable_amp_obs needs motion_lib: the reset state, the AMP window's history and the demonstration windows "
                             "all come from the motion library (humanoid_amp.py:215-284, 447-488, 535-563)")
        state_init = env.get("stateInit", "Random")
        if state_init not in ("Random", "Start"):
            raise NotImplementedError(f"{name}: stateInit {state_init!r}: Random and Start are built (Default / Hybrid need the simulator's "
                                      "default pose, humanoid_amp.py:447-505)")
        for key in ("has_shape_obs_disc", "has_weight_obs_disc"):
            if env.get(key, False):
                raise NotImplementedError(f"{name}: {key}: the downstream tasks carry no shape rows (humanoid_shapes / humanoid_limb_and_weights, "
                                          "humanoid.py:739-878; humanoid_amp.py:311-314, 963-966): only HumanoidIm appends them to the AMP frame")
        if getattr(lib, "num_bodies", self.num_bodies) != self.num_bodies:
            raise ValueError(f"{name}: the motion library has {lib.num_bodies} bodies, the task {self.num_bodies}")
        if getattr(self.sim, "dof_pos", None) is None:
            raise ValueError(f"{name}: enable_amp_obs needs the simulator's dof_pos tensor")
        self._state_init_random = state_init != "Start"
        self._amp_gen = torch.Generator(device=dev)
        self._amp_gen.manual_seed(int(env.get("amp_seed", 4242)))
        self._sampled_motion_ids = torch.zeros(n, dtype=torch.int64, device=dev)
        self._motion_start_times = torch.zeros(n, device=dev)
        self._reset_ref_motion_ids = self._reset_ref_motion_times = None             # the draws of the last reset, every env's (humanoid_amp.py:481-483)
        self._zero_times = torch.zeros(n, device=dev)
        self._demo_bufs, self._last_demo = {}, None
        self._amp = w = AmpWindow(env, num_envs=n, device=dev, skeleton=syn.skeleton("smpl"), local_root_obs=self._local_root_obs,
                                  upright=self._has_upright_start, amp_obs_v=check_amp_options(env, lib))
        self._num_amp_obs_steps, self._num_amp_obs_per_step, self._amp_obs_buf, self._amp_obs_space = w.num_steps, w.per_step, w.buf, w.space

    def get_num_amp_obs(self):
        return self._amp.num_obs()

    def set_amp_obs_sink(self, rows):
        """The NEXT post_physics_step writes its finished AMP window into ``rows`` as well and hands that view out as extras['amp_obs']."""
        self._amp.set_sink(rows)

    def fetch_amp_obs_demo(self, num_samples):
        """humanoid_amp.py:215-284: ``num_samples`` AMP windows of reference motion, drawn with the task's own generator."""
        out, self._demo_bufs, ids, t0 = self._amp.fetch_demo(num_samples, self._motion_lib, self.dt, self._amp_gen, bufs=self._demo_bufs)
        self._last_demo = (ids, t0)
        return out

    def _ref_state_kwargs(self, mask=None):
        """The transform arguments of ops.task_ref_state_init beside ``transform`` (the terrain task adds its location and height field);
        ``mask``: the envs being reset."""
        return {}

    def _reset_ref_state_init(self, mask):
        """_reset_ref_state_init (humanoid_amp.py:468-488): a clip and a start time per env (sample_motions / _sample_time draw for every env;
        the masked ones use theirs), then the simulator's state, the start time, the motion id and the episode words in one launch."""
        lib, n = self._motion_lib, self.num_envs
        ids = lib.sample_motions(n, generator=self._amp_gen)
        times = lib.sample_time_interval(ids, generator=self._amp_gen) if self._state_init_random else self._zero_times
        self._reset_ref_motion_ids, self._reset_ref_motion_times = ids, times
        sim = self.sim
        ops.task_ref_state_init(lib, ids, times, mask, sim.rigid_body_state, sim.dof_pos, sim.dof_vel, self._motion_start_times, self._sampled_motion_ids,
                                clears=(self.progress_buf, self.reset_buf, self._terminate_buf), transform=self.REF_STATE_TRANSFORM,
                                upright=self._has_upright_start, **self._ref_state_kwargs(mask))
        if hasattr(sim, "on_reset"):
            sim.on_reset(mask)

    # ---- sizes
    def _task_obs_width(self, env):
        return ops._lib.load().pulse_task_obs_size({"speed": 1, "reach": 2, "strike": 3}[self.TASK])

    def _reward_raw_width(self):
        return 2 if self.power_reward else 1

    def get_obs_size(self):
        return self.num_obs

    def get_self_obs_size(self):
        return self._self_obs_size

    def get_task_obs_size(self):
        return self._task_obs_size

    def get_running_mean_size(self):
        return (self.num_obs,)

    def get_task_obs_size_detail(self):
        return {}

    # ---- per-task hooks
    def _task_kwargs(self):
        raise NotImplementedError

    def _reset_task(self, mask):
        raise NotImplementedError

    def _task_due(self):
        raise NotImplementedError

    def _update_task(self):
        self._reset_task(self._task_due())                       # masked: envs whose change step has come (no nonzero() read-back)

    def _rand(self, *shape):
        return torch.rand(*shape, device=self.device, generator=self._task_gen)

    def _randint(self, low, high):
        return torch.randint(low, high, (self.num_envs,), device=self.device, dtype=torch.int64, generator=self._task_gen)

    # ---- step phases (humanoid.py:1077-1110, 1315-1331; humanoid_amp_task.py:68-83)
    def _task_step(self, what, env_mask=None):
        kw = self._task_kwargs()
        return ops.task_step(self.TASK, self.sim.rigid_body_state, what=what, prev_root_pos=self._prev_root_pos, dt=self.dt,
                             contact_forces=self.sim.contact_forces, contact_body_ids=self._contact_body_ids,
                             termination_heights=self._termination_heights, progress=self.progress_buf,
                             max_episode_length=float(self.max_episode_length), enable_early_termination=self._enable_early_termination,
                             dof_force=self.sim.dof_force if self.power_reward else None, dof_vel=self.sim.dof_vel if self.power_reward else None,
                             power_coef=self.power_coefficient, power_reward=self.power_reward, obs=self._obs_store, obs_offset=self._self_obs_size,
                             rew=self.rew_buf, rew_raw=self.reward_raw, reset=self.reset_buf, terminate=self._terminate_buf, env_mask=env_mask, **kw)

    def _compute_observations(self, env_mask=None):
        ops.im_step(self.sim.rigid_body_state, what=PULSE_IM_SELF_OBS, local_root_obs=self._local_root_obs, root_height_obs=self._root_height_obs,
                    upright=self._has_upright_start, obs=self._obs_store, obs_cols=self._self_obs_size, env_mask=env_mask)
        if self._enable_task_obs:
            self._task_step(TASK_OBS, env_mask=env_mask)

    def set_action_clip(self, clip):
        """VecTaskPythonWrapper hands its clip_actions down: the clamp runs inside the actuation launch."""
        self._actuation.clip = float(clip)
        return True

    def pre_physics_step(self, actions):
        self._prev_root_pos.copy_(self.sim.rigid_body_state[:, 0, 0:3])                 # humanoid_speed.py:72-75
        # humanoid.py:1226-1247, 1392-1394: self.actions (the clamped copy) and offset + scale * action, frozen joints at 0, in one launch
        self.actions, pd_tar = self._actuation(actions)
        self.sim.set_dof_position_target_tensor(pd_tar)
        self._update_task()          # HumanoidAMPTask.pre_physics_step (humanoid_amp_task.py:57-59): BEFORE progress_buf advances

    def step(self, actions):
        self.pre_physics_step(actions)
        self.sim.simulate_and_refresh()                                                  # Isaac Gym: OUT OF SCOPE
        self.post_physics_step()

    def post_physics_step(self):
        self.progress_buf += 1
        # reward -> reset (one launch), then the observation row for the next step (humanoid.py:1322-1325)
        self._task_step(TASK_REWARD | TASK_RESET)
        raw = self.reward_raw
        if self.power_usage_reward:
            raw = self._add_power_usage_reward(raw)
        self._compute_observations()
        self.extras["terminate"] = self._terminate_buf
        self.extras["reward_raw"] = raw
        if self._enable_amp_obs:                      # HumanoidAMP.post_physics_step (humanoid_amp.py:194-210)
            self.extras["amp_obs"] = self._amp.step(self.sim)

    def _add_power_usage_reward(self, raw):
        """humanoid_speed.py:225-238 / humanoid_strike.py:186-198, statement for statement on the kernel's reward (torch ops, as in the
        reference: the option is off in every shipped config).  The speed task appends the term to reward_raw, the strike task does not."""
        power_all = torch.abs(torch.multiply(self.sim.dof_force, self.sim.dof_vel)).reshape(-1, self._dof_size // 3, 3)
        left_power = power_all[:, self._left_idx].reshape(self.num_envs, -1).sum(dim=-1)
        right_power = power_all[:, self._right_idx].reshape(self.num_envs, -1).sum(dim=-1)
        self.power_acc[:, 0] += left_power
        self.power_acc[:, 1] += right_power
        pur = self.power_acc / (self.progress_buf + 1)[:, None]
        pur = -self.power_usage_coefficient * (pur[:, 0] - pur[:, 1]).abs()
        pur = torch.where(self.progress_buf <= 3, torch.zeros_like(pur), pur)           # (pur[progress <= 3] = 0 without a host read)
        self.rew_buf += pur
        return torch.cat([raw, pur[:, None]], dim=-1) if self.TASK == "speed" else raw

    def reset(self, env_ids=None):
        if env_ids is None:
            mask = torch.ones(self.num_envs, dtype=torch.bool, device=self.device)
        else:
            if not isinstance(env_ids, torch.Tensor):
                if len(env_ids) == 0:
                    return
                env_ids = torch.tensor(env_ids, dtype=torch.int64, device=self.device)
            if env_ids.numel() == 0:
                return
            mask = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
            mask[env_ids] = True
        self.reset_masked(mask)

    def reset_masked(self, mask):
        """_reset_envs (humanoid.py:574-587) + HumanoidAMPTask._reset_envs (task reset before the observation)."""
        if self._enable_amp_obs:
            self._reset_ref_state_init(mask)                    # state from the motion; progress / reset / terminate cleared in the launch
        else:
            keep = ~mask
            self.sim.set_env_states_masked(mask)
            self.progress_buf.mul_(keep)
            self.reset_buf.mul_(keep)
            self._terminate_buf.mul_(keep)
        if self.power_usage_reward and self.TASK == "speed":
            self.power_acc.masked_fill_(mask[:, None], 0.0)     # HumanoidSpeed._reset_ref_state_init (humanoid_speed.py:247-249); the strike task never clears it
        self._reset_task(mask)
        self._compute_observations(env_mask=mask)
        if self._enable_amp_obs:                                # _init_amp_obs (humanoid_amp.py:519-563): current frame, then the clip's past
            self._amp.init(self.sim, mask, lib=self._motion_lib, motion_ids=self._sampled_motion_ids, start_times=self._motion_start_times, dt=self.dt)


class HumanoidSpeed(HumanoidTask):
    TASK = "speed"
    REF_STATE_TRANSFORM = "remove_heading"          # humanoid_speed.py:251-270

    def __init__(self, cfg, sim, device="cuda:0", motion_lib=None):
        super().__init__(cfg, sim, device, motion_lib)
        env = cfg.get("env", cfg)
        self._tar_speed_min, self._tar_speed_max = float(env.get("tarSpeedMin", 0.0)), float(env.get("tarSpeedMax", 5.0))
        self._speed_change_steps_min = int(env.get("speedChangeStepsMin", 100))
        self._speed_change_steps_max = int(env.get("speedChangeStepsMax", 200))
        self._speed_change_steps = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)
        self._tar_speed = torch.ones(self.num_envs, device=self.device)

    def _task_due(self):
        return self.progress_buf >= self._speed_change_steps                               # humanoid_speed.py:153-160

    def _reset_task(self, mask):
        """humanoid_speed.py:162-171 for the masked envs."""
        tar = (self._tar_speed_max - self._tar_speed_min) * self._rand(self.num_envs) + self._tar_speed_min
        steps = self._randint(self._speed_change_steps_min, self._speed_change_steps_max)
        torch.where(mask, tar, self._tar_speed, out=self._tar_speed)
        torch.where(mask, self.progress_buf + steps, self._speed_change_steps, out=self._speed_change_steps)

    def _task_kwargs(self):
        return {"tar_speed": self._tar_speed}


class HumanoidReach(HumanoidTask):
    TASK = "reach"
    REF_STATE_TRANSFORM = "zero_xy"                 # humanoid_reach.py:46-49

    def __init__(self, cfg, sim, device="cuda:0", motion_lib=None):
        super().__init__(cfg, sim, device, motion_lib)
        env = cfg.get("env", cfg)
        self._tar_change_steps_min, self._tar_change_steps_max = int(env.get("tarChangeStepsMin", 100)), int(env.get("tarChangeStepsMax", 200))
        self._tar_dist_max = float(env.get("tarDistMax", 1.0))
        self._tar_height_min, self._tar_height_max = float(env.get("tarHeightMin", 0.6)), float(env.get("tarHeightMax", 1.6))
        self._reach_body_id = syn.SMPL_BODY_NAMES.index(env.get("reachBodyName", "R_Hand"))
        self._tar_change_steps = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)
        self._tar_pos = torch.zeros(self.num_envs, 3, device=self.device)

    def _task_due(self):
        return self.progress_buf >= self._tar_change_steps                                # humanoid_reach.py:122-127

    def _reset_task(self, mask):
        """humanoid_reach.py:129-142 for the masked envs."""
        r = self._rand(self.num_envs, 3)
        r[:, 0:2] = self._tar_dist_max * (2.0 * r[:, 0:2] - 1.0)
        r[:, 2] = (self._tar_height_max - self._tar_height_min) * r[:, 2] + self._tar_height_min
        steps = self._randint(self._tar_change_steps_min, self._tar_change_steps_max)
        torch.where(mask[:, None], r, self._tar_pos, out=self._tar_pos)
        torch.where(mask, self.progress_buf + steps, self._tar_change_steps, out=self._tar_change_steps)

    def _task_kwargs(self):
        return {"tar_pos": self._tar_pos, "reach_body_id": self._reach_body_id}


class HumanoidStrike(HumanoidTask):
    TASK = "strike"
    REF_STATE_TRANSFORM = "zero_xy"                 # humanoid_strike.py:147-150

    def __init__(self, cfg, sim, device="cuda:0", motion_lib=None):
        super().__init__(cfg, sim, device, motion_lib)
        env = cfg.get("env", cfg)
        self._tar_dist_min, self._tar_dist_max = float(env.get("tarDistMin", 0.5)), float(env.get("tarDistMax", 10.0))
        self._near_dist, self._near_prob = float(env.get("nearDist", 1.5)), float(env.get("nearProb", 0.5))
        strike = env.get("strikeBodyNames", ["R_Hand", "R_Wrist", "R_Elbow"])
        self._strike_body_ids = torch.tensor([syn.SMPL_BODY_NAMES.index(b) for b in strike], dtype=torch.int32, device=self.device)
        self._target_states = sim.target_states                                           # (N, 13) root state of the target object

    def _task_due(self):
        return torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)           # the target only moves at episode reset

    def _reset_task(self, mask):
        """_reset_target, humanoid_strike.py:125-145 for the masked envs."""
        n = self.num_envs
        near = self._rand(n) < self._near_prob
        dist_max = torch.where(near, torch.full((n,), self._near_dist, device=self.device), torch.full((n,), self._tar_dist_max, device=self.device))
        dist = (dist_max - self._tar_dist_min) * self._rand(n) + self._tar_dist_min
        theta = 2 * math.pi * self._rand(n)
        rot_theta = 2 * math.pi * self._rand(n)
        root = self.sim.rigid_body_state[:, 0]
        new = torch.zeros(n, 13, device=self.device)
        new[:, 0] = dist * torch.cos(theta) + root[:, 0]
        new[:, 1] = dist * torch.sin(theta) + root[:, 1]
        new[:, 2] = 0.9
        new[:, 5], new[:, 6] = torch.sin(rot_theta / 2), torch.cos(rot_theta / 2)            # quat_from_angle_axis(theta, z)
        torch.where(mask[:, None], new, self._target_states, out=self._target_states)

    def _task_kwargs(self):
        return {"tar_states": self._target_states, "tar_contact_forces": self.sim.target_contact_forces, "strike_body_ids": self._strike_body_ids}


class HumanoidTraj(HumanoidTask):
    """HumanoidTraj (phc/env/tasks/humanoid_traj.py:22-211): follow a random 2-D trajectory (TrajGenerator, phc/utils/traj_generator.py);
    task observation = numTrajSamples (10) future trajectory points in the heading frame, reward exp(-2 |root - target|^2), reset when
    fallen or more than fail_dist (4 m) off the trajectory.  One launch of pulse_traj_step per phase; trajectories are regenerated for the
    envs being reset by pulse_traj_generate from six uniform draws taken in the reference's order."""
    TASK = "traj"
    TERRAIN_OBS = False
    CROWD = False                                   # the reference's HumanoidTraj never looks at the crowd keys; its terrain task does

    def __init__(self, cfg, sim, device="cuda:0", motion_lib=None):
        from .humanoid_im import check_humanoid_options
        check_humanoid_options(cfg, type(self).__name__)     # before the height points go to the device
        env = cfg.get("env", cfg)
        self._num_traj_samples = int(env.get("numTrajSamples", 10))
        self._traj_sample_timestep = float(env.get("trajSampleTimestep", 0.5))
        self.terrain_obs = bool(env.get("terrain_obs", self.TERRAIN_OBS))
        self._height_points = self._center_points = self._heightsamples = None
        self._terrain = self._sim_terrain(env, sim)                                          # before anything goes to the device
        if self.terrain_obs:
            if env.get("terrain_obs_type", "square") != "square":
                raise NotImplementedError("terrain_obs_type 'square' (env_pulse_terrain.yaml) is built; 'fov' / 'square_fov' are viewer-era variants")
            self._height_points = syn.square_height_points(float(env.get("sensor_extent", 2)), int(env.get("sensor_res", 32))).to(device)
        self._read_crowd_options(env, sim.num_envs)
        super().__init__(cfg, sim, device, motion_lib)
        dev = self.device
        self._speed_min, self._speed_max = float(env.get("speedMin", 0.0)), float(env.get("speedMax", 3.0))
        self._accel_max, self._sharp_turn_prob = float(env.get("accelMax", 2.0)), float(env.get("sharpTurnProb", 0.02))
        self._fail_dist = 4.0                                                            # humanoid_traj.py:30
        self._num_verts, self._dtheta_max = 101, 2.0                                     # _build_traj_generator (:105-113)
        self._episode_dur = self.max_episode_length * self.dt
        self._traj_verts = torch.zeros(self.num_envs, self._num_verts, 3, device=dev)
        self.fuzzy_target = bool(env.get("fuzzy_target", False))
        self._sensor_body = 0
        if self.terrain_obs:
            self._center_points = syn.center_height_points().to(dev)
            self._use_center_height = bool(env.get("use_center_height", False))
            self._sensor_body = syn.SMPL_BODY_NAMES.index("Head") if env.get("terrain_obs_root", "head") == "head" else 0
            terrain_type = env.get("terrain", {}).get("terrainType", "trimesh")
            if terrain_type == "none":
                raise NameError("Can't measure height with terrain type 'none'")            # get_heights (:744-745)
            if terrain_type != "plane":
                hs = getattr(sim, "heightsamples", None) if self._terrain is None else self._terrain.heightsamples
                self._heightsamples = (hs if hs is not None else syn.synthetic_height_field()).to(dev).contiguous()
            self._horizontal_scale, self._vertical_scale, self.height_meas_scale = 0.1, 0.005, 5.0    # Terrain.__init__ (:1121-1122), :69
        self._init_crowd(dev)

    def _sim_terrain(self, env, sim):
        """``sim.terrain`` (env/terrain.py: the map and its walkable field) when the simulator publishes one and the task can walk on it; a
        terrain the task would have to ignore raises instead of falling back to the uniform draw without a word."""
        terrain = getattr(sim, "terrain", None)
        if terrain is None:
            return None
        name, terrain_type = type(self).__name__, env.get("terrain", {}).get("terrainType", "trimesh")
        if not self.terrain_obs:
            raise ValueError(f"{name}: the simulator publishes a terrain, but terrain_obs is off: this task never looks at a map "
                             "(HumanoidTraj has none, phc/env/tasks/humanoid_traj.py)")
        if terrain_type == "plane":
            raise ValueError(f"{name}: the simulator publishes a terrain, but terrainType is 'plane': the reference builds no map there "
                             "(Terrain.__init__ returns first, phc/env/tasks/humanoid_pedestrian_terrain.py:1119-1120)")
        hs = getattr(sim, "heightsamples", None)
        if hs is not None and tuple(hs.shape) != tuple(terrain.heightsamples.shape):
            raise ValueError(f"{name}: the simulator publishes a terrain of {tuple(terrain.heightsamples.shape)} cells and heightsamples of "
                             f"{tuple(hs.shape)}: which map the humanoids walk on is ambiguous")
        return terrain

    # ---- crowd variant (humanoid.py:256-261; humanoid_pedestrian_terrain.py:253-293, 385-439, 718-772, 1200-1276, 1700-1753)
    def _read_crowd_options(self, env, num_envs):
        """divide_group / group_obs / disable_group_obs / num_env_group / velocity_map.  ``flags.divide_group``, the global the reference
        also consults in get_heights (:749), is False in training and treated as such."""
        on = self.CROWD
        self._divide_group = on and bool(env.get("divide_group", False))
        self._group_obs = on and bool(env.get("group_obs", False))
        self._disable_group_obs = on and bool(env.get("disable_group_obs", False))
        self.velocity_map = on and self.terrain_obs and bool(env.get("velocity_map", False))
        self._group_num_people = 0
        if self._divide_group:
            g = self._group_num_people = min(int(env.get("num_env_group", 128)), num_envs)       # humanoid.py:259
            if g < 1 or num_envs % g != 0:
                raise ValueError(f"divide_group: num_envs = {num_envs} is not a multiple of the group size {g} (num_env_group): the reference's "
                                 "group ids, arange(num_envs / G).repeat(G) (phc/env/tasks/humanoid.py:260), have no meaning there")
            if self._group_obs and g < 6:
                raise ValueError(f"group_obs: group size {g} < 6: compute_group_observation takes the 6 smallest group distances "
                                 "(torch.topk, phc/env/tasks/humanoid_pedestrian_terrain.py:1724)")
        self._people_obs = self._divide_group and self._group_obs                        # the 165-float neighbour block (:264-267, 431-437)
        # people stamped into the height map (get_heights :749): only where there is a height map to stamp
        self._stamps = self._divide_group and not self._group_obs and not self._disable_group_obs and self.terrain_obs
        terrain_type = env.get("terrain", {}).get("terrainType", "trimesh")
        if self.velocity_map and terrain_type == "plane":
            raise NotImplementedError("velocity_map on terrainType 'plane': get_heights returns (num_envs, num_height_points) zeros there "
                                      "(phc/env/tasks/humanoid_pedestrian_terrain.py:721-725) and _compute_task_obs then views them as "
                                      "(num_envs, -1, 3) (:418-421) or concatenates a block a third as wide as get_task_obs_size says "
                                      "(:260-263): the reference cannot run this combination")
        # on a plane get_heights returns zeros BEFORE it looks at the root points (:721-725): stamps change nothing there
        self._crowd_heights = (self._stamps or self.velocity_map) and terrain_type != "plane"

    def _init_crowd(self, dev):
        self._owner = self._stamp_cells = None
        if self._stamps and self._crowd_heights:
            rows, cols = self._heightsamples.shape
            self._owner = torch.zeros(self.num_envs // self._group_num_people, rows, cols, dtype=torch.int32, device=dev)
            self._stamp_cells = torch.full((self.num_envs, 200), -1, dtype=torch.int32, device=dev)

    def _height_block_width(self):
        if self._height_points is None:
            return 0
        return self._height_points.shape[0] * (3 if self.velocity_map else 1)

    def _task_obs_width(self, env):
        w = 2 * self._num_traj_samples + self._height_block_width()                      # get_task_obs_size (:253-270)
        if self._people_obs:
            w += 5 * 11 * 3
        return w

    def _reward_raw_width(self):
        return 2                                                                         # [location reward, power reward] (:890)

    def get_task_obs_size_detail(self):
        d = {"traj": 2 * self._num_traj_samples}                                         # get_task_obs_size_detail (:273-290)
        if self.terrain_obs:
            d["heightmap_velocity" if self.velocity_map else "heightmap"] = self._height_block_width()
        if self._people_obs:
            d["people"] = 5 * 11 * 3
        return d

    def _task_due(self):
        return None

    def _update_task(self):
        return                                                                           # trajectories only change at episode reset

    def _reset_task(self, mask):
        """HumanoidTraj._reset_task (:145-150) -> TrajGenerator.reset for the masked envs."""
        # This runs on EVERY rollout step (the done mask lives on the device): all draws of a call come from ONE uniform launch into a persistent
        # buffer (four (N, V - 1) blocks + two (N,) rows), the sharp-turn Bernoulli is a compare of its block (five RNG launches and
        # six allocations per step before).  The reference draws len(env_ids) rows per reset: the RNG streams were never comparable.
        n, v = self.num_envs, self._num_verts
        blk = n * (v - 1)
        buf = getattr(self, "_traj_draws", None)
        if buf is None or buf.numel() != 4 * blk + 2 * n:
            buf = self._traj_draws = torch.empty(4 * blk + 2 * n, device=self.device)
            self._traj_sharp = torch.empty(n, v - 1, dtype=torch.bool, device=self.device)
        buf.uniform_(generator=self._task_gen)
        u_dtheta, u_sharp, u_dspeed, u_turn = (buf[i * blk:(i + 1) * blk].view(n, v - 1) for i in range(4))
        u_heading, u_speed0 = buf[4 * blk:4 * blk + n], buf[4 * blk + n:]
        sharp_mask = torch.lt(u_turn, self._sharp_turn_prob, out=self._traj_sharp)
        ops.traj_generate(self.sim.rigid_body_state, self._traj_verts, u_dtheta, u_sharp, sharp_mask, u_heading, u_dspeed, u_speed0,
                          episode_dur=self._episode_dur, dtheta_max=self._dtheta_max, speed_min=self._speed_min, speed_max=self._speed_max,
                          accel_max=self._accel_max, env_mask=mask)

    def _task_step(self, what, env_mask=None):
        terrain = {}
        if self.terrain_obs and not self._crowd_heights:
            terrain = dict(heightsamples=self._heightsamples, horizontal_scale=self._horizontal_scale, vertical_scale=self._vertical_scale,
                           height_points=self._height_points, sensor_body=self._sensor_body, center_points=self._center_points,
                           use_center_height=self._use_center_height, height_meas_scale=self.height_meas_scale)
        out = ops.traj_step(self.sim.rigid_body_state, self._traj_verts, self.progress_buf, what=what, dt=self.dt, episode_dur=self._episode_dur,
                             num_samples=self._num_traj_samples, sample_timestep=self._traj_sample_timestep, upright=self._has_upright_start,
                             dof_force=self.sim.dof_force, dof_vel=self.sim.dof_vel, power_coef=self.power_coefficient, power_reward=self.power_reward,
                             fuzzy_target=self.fuzzy_target, contact_forces=self.sim.contact_forces, contact_body_ids=self._contact_body_ids,
                             termination_heights=self._termination_heights, max_episode_length=float(self.max_episode_length),
                             fail_dist=self._fail_dist, enable_early_termination=self._enable_early_termination, terrain_reset=self.terrain_obs,
                             obs=self._obs_store, obs_offset=self._self_obs_size, rew=self.rew_buf, rew_raw=self.reward_raw, reset=self.reset_buf,
                             terminate=self._terminate_buf, env_mask=env_mask, **terrain)
        if (what & TASK_OBS) and (self._crowd_heights or self._people_obs):
            self._crowd_obs(env_mask)
        return out

    def _crowd_obs(self, env_mask):
        """[height block | people block] behind the trajectory samples pulse_traj_step wrote (it ran without a height sensor when the height
        block is the crowd kernels').  Stamps and neighbours come from EVERY env's state; only the rows of ``env_mask`` are written, as the
        reference indexes the whole-group result by env_ids (:433-435)."""
        rb, col = self.sim.rigid_body_state, self._self_obs_size + 2 * self._num_traj_samples
        if self._crowd_heights:
            if self._stamps:
                ops.crowd_stamp(rb, self._group_num_people, self._owner, self._stamp_cells, horizontal_scale=self._horizontal_scale)
            ops.crowd_heights(rb, self._heightsamples, self._height_points, group_size=self._group_num_people, owner=self._owner,
                              velocity_map=self.velocity_map, upright=self._has_upright_start, sensor_body=self._sensor_body,
                              center_points=self._center_points, use_center_height=self._use_center_height,
                              horizontal_scale=self._horizontal_scale, vertical_scale=self._vertical_scale,
                              height_meas_scale=self.height_meas_scale, obs=self._obs_store, obs_offset=col, env_mask=env_mask)
        if self._people_obs:
            ops.crowd_group_obs(rb, self._group_num_people, upright=self._has_upright_start, obs=self._obs_store,
                                obs_offset=col + self._height_block_width(), env_mask=env_mask)


class HumanoidPedestrianTerrain(HumanoidTraj):
    """HumanoidPedestrianTerrain (phc/env/tasks/humanoid_pedestrian_terrain.py:31-890; env_pulse_terrain.yaml): the trajectory task over a height
    field -- the task observation gains the 32 x 32 height map under the head (:384-440), a fall is a summed non-foot contact force above
    50 N (:1476-1531), the reward keeps a power term (:871-890).

    The map: when the simulator publishes ``sim.terrain`` (env/terrain.py:Terrain -- the reference's geometry, tile layout, obstacle field
    of the 'poles' tiles with its 3-step dilation, table of valid start cells), its height field is the task's and every reset location is
    drawn from the valid cells (Terrain.sample_valid_locations, :531, 1175-1189).  Without one the map is ``sim.heightsamples`` or a
    synthetic height field, and reset locations are uniform over its interior.  Not built: the sub-terrain generators
    (isaacgym.terrain_utils; Terrain takes them as plug-ins), convert_heightfield_to_trimesh and anything PhysX, MeshTerrain (:975-1112),
    the flags.fixed / flags.server_mode placements (:535-549).

    Crowd variant (no shipped config enables it; configs.crowd_env): ``divide_group`` partitions the envs into contiguous groups of
    min(num_env_group, num_envs) (humanoid.py:256-261).  With ``group_obs`` the task observation gains the 165-float 'people' block,
    the 5 nearest other members of the env's group (compute_group_observation, :1700-1753); without it (and without
    ``disable_group_obs``) every person is stamped into its group's copy of the height map as a 10 x 20 footprint 1.7 m high
    (get_heights :749-761, sample_height_points :1207-1259).  ``velocity_map``, with or without groups, makes the height block
    [h, vx, vy] per point ('heightmap_velocity', :1236-1276).  In these modes pulse_traj_step runs without its height sensor and the
    kernels of csrc/crowd_obs.hip write [height block | people block] behind the trajectory samples.  Not built, and rejected where they
    would be used: the 'people' point-net branch of amp_sept (learning/network_sept.py -- the flat networks read the wider observation as
    it is), _compute_flip_task_obs (mirroring augmentation, :442-478), Isaac collision groups per env group (humanoid.py:919) and the 'fov'
    sensor types."""
    TERRAIN_OBS = True
    CROWD = True
    REF_STATE_TRANSFORM = "terrain"                 # humanoid_pedestrian_terrain.py:527-589

    def _ref_state_kwargs(self, mask=None):
        """The new location of every env (:531) and the height field the root is lifted over (:553-563).  With a Terrain: a draw from its
        valid start cells for the envs of ``mask`` (Terrain.sample_into; the rows of the other envs keep what they held).  Without: uniform
        over the interior of the height field, a sensor reach from its edges.  Both from the generator the motions are drawn with."""
        hs = self._heightsamples
        if self._terrain is not None:
            xy = getattr(self, "_new_root_xy", None)
            if xy is None:
                xy = self._new_root_xy = torch.zeros(self.num_envs, 2, device=self.device)
            self._terrain.sample_into(xy, mask, self._amp_gen)
            return dict(new_root_xy=xy, heightsamples=hs, horizontal_scale=self._horizontal_scale, vertical_scale=self._vertical_scale,
                        center_points=self._center_points)
        rows, cols = hs.shape if hs is not None else (260, 300)                   # terrainType 'plane': the extent of the synthetic field
        scale = getattr(self, "_horizontal_scale", 0.1)
        extent = torch.tensor([rows * scale, cols * scale], device=self.device)
        margin = 3.0
        xy = margin + torch.rand(self.num_envs, 2, device=self.device, generator=self._amp_gen) * (extent - 2 * margin)
        self._new_root_xy = xy
        kw = {"new_root_xy": xy}
        if hs is not None:
            kw.update(heightsamples=hs, horizontal_scale=self._horizontal_scale, vertical_scale=self._vertical_scale, center_points=self._center_points)
        return kw


class _ZMixin(HumanoidZ):
    """HumanoidSpeedZ / ReachZ / StrikeZ (humanoid_speed.py:290-304 ...): the action is the 32-d latent of a frozen PULSE decoder."""

    def _init_z(self, cfg):
        env = cfg.get("env", cfg)
        self._embedding_size = int(env.get("embedding_size", 32))
        self.num_actions = self._embedding_size
        self._read_z_options(env)

    def step(self, action_z):
        self.action_z = action_z
        actions = self.compute_z_actions(action_z)
        self.pre_physics_step(actions)
        self.sim.simulate_and_refresh()
        self.post_physics_step()


class HumanoidSpeedZ(_ZMixin, HumanoidSpeed):
    def __init__(self, cfg, sim, device="cuda:0", motion_lib=None):
        super().__init__(cfg, sim, device, motion_lib)
        self._init_z(cfg)


class HumanoidReachZ(_ZMixin, HumanoidReach):
    def __init__(self, cfg, sim, device="cuda:0", motion_lib=None):
        super().__init__(cfg, sim, device, motion_lib)
        self._init_z(cfg)


class HumanoidStrikeZ(_ZMixin, HumanoidStrike):
    def __init__(self, cfg, sim, device="cuda:0", motion_lib=None):
        super().__init__(cfg, sim, device, motion_lib)
        self._init_z(cfg)


class HumanoidPedestrianTerrainZ(_ZMixin, HumanoidPedestrianTerrain):
    """humanoid_pedestrian_terrain.py:957-972: the terrain task driven through a frozen PULSE decoder (learning=pulse_z_terrain)."""

    def __init__(self, cfg, sim, device="cuda:0", motion_lib=None):
        super().__init__(cfg, sim, device, motion_lib)
        self._init_z(cfg)


class SyntheticTaskSim:
    """Physics stand-in for the downstream tasks: a bank of recorded frames (rigid bodies with a drifting root, sparse contact
    forces, a target object) replayed one per control step.  Actions are accepted and ignored, exactly like RecordedSim."""

    def __init__(self, num_envs, frames, device, seed=1234, rank=0, fall_rate=0.01, xy_offset=(0.0, 0.0), dof_pos_bank=False, dof_limits=None,
                 terrain=None):
        g = syn.make_generator(seed + 31, rank)
        n, j, f = num_envs, syn.NUM_BODIES, frames
        self.num_envs, self.frames, self.frame = n, f, 0
        rb = torch.stack([syn.rigid_body_state(g, n) for _ in range(f)])
        drift = torch.cumsum(0.05 * torch.randn(f, n, 1, 3, generator=g), dim=0)
        drift[..., 2] = 0
        rb[..., 0:3] += drift
        rb[..., 0] += xy_offset[0]                                                             # e.g. into the interior of a height field
        rb[..., 1] += xy_offset[1]
        contact = torch.zeros(f, n, j, 3)
        fell = torch.rand(f, n, generator=g) < fall_rate
        contact[..., 9, 2] = fell.float() * 200.0                                          # torso contact
        rb[..., 9, 2] = torch.where(fell, torch.full_like(rb[..., 9, 2], 0.05), rb[..., 9, 2])
        self.bank = {"rb": rb.to(device), "contact": contact.to(device), "dof_force": (50.0 * torch.randn(f, n, syn.NUM_DOF, generator=g)).to(device),
                     "dof_vel": torch.randn(f, n, syn.NUM_DOF, generator=g).to(device),
                     "tar_contact": (30.0 * torch.randn(f, n, 3, generator=g)).to(device)}
        self.rigid_body_state = self.bank["rb"][0].clone()
        self.contact_forces = self.bank["contact"][0].clone()
        self.dof_force, self.dof_vel = self.bank["dof_force"][0].clone(), self.bank["dof_vel"][0].clone()
        self.dof_pos = torch.zeros(n, syn.NUM_DOF, device=device)
        if dof_pos_bank:
            # joint angles per frame for the AMP frame (enable_amp_obs), from a generator of their own: every other tensor is the same draw
            # for draw with and without them
            self.bank["dof_pos"] = (0.5 * torch.randn(f, n, syn.NUM_DOF, generator=syn.make_generator(seed + 57, rank))).to(device)
            self.dof_pos.copy_(self.bank["dof_pos"][0])
        self.target_states = torch.zeros(n, 13, device=device)
        self.target_states[:, 6] = 1.0
        self.target_contact_forces = self.bank["tar_contact"][0].clone()
        self.pd_targets = None
        if terrain is not None:
            self.terrain = terrain                                                         # env/terrain.py:Terrain, read by the terrain task
        from .sim import publish_dof_limits
        publish_dof_limits(self, dof_limits, syn.NUM_DOF, device)

    def set_dof_position_target_tensor(self, pd_tar):
        self.pd_targets = pd_tar

    def simulate_and_refresh(self):
        self.frame = (self.frame + 1) % self.frames
        f, b = self.frame, self.bank
        self.rigid_body_state.copy_(b["rb"][f])
        self.contact_forces.copy_(b["contact"][f])
        self.dof_force.copy_(b["dof_force"][f])
        self.dof_vel.copy_(b["dof_vel"][f])
        self.target_contact_forces.copy_(b["tar_contact"][f])
        if "dof_pos" in b:
            self.dof_pos.copy_(b["dof_pos"][f])

    def set_env_states_masked(self, mask):
        return


TASKS = {"HumanoidSpeed": HumanoidSpeed, "HumanoidReach": HumanoidReach, "HumanoidStrike": HumanoidStrike,
         "HumanoidSpeedZ": HumanoidSpeedZ, "HumanoidReachZ": HumanoidReachZ, "HumanoidStrikeZ": HumanoidStrikeZ,
         "HumanoidTraj": HumanoidTraj, "HumanoidPedestrianTerrain": HumanoidPedestrianTerrain,
         "HumanoidPedestrianTerrainZ": HumanoidPedestrianTerrainZ}
