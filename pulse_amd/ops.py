"""Tensor-level wrappers over the C ABI, named after the reference functions they replace.

Every function takes ``torch`` tensors that already live on the GPU, checks
dtype / layout, and enqueues the HIP kernel on torch's CURRENT stream through
``libpulse_hip.so`` (PyTorch is only the allocator / stream provider here).
There is no fallback: CPU tensors are rejected and a missing library raises.

Reference mapping (paths relative to the reference root):
  quat_mul, quat_conjugate                 isaacgym.torch_utils (3P)
  my_quat_rotate ... calc_heading_quat_inv phc/utils/torch_utils.py:45-240
  compute_humanoid_observations_smpl_max   phc/env/tasks/humanoid.py:1675-1731
  compute_imitation_observations_v6 / _v7  phc/env/tasks/humanoid_im.py:1328-1413
  compute_imitation_reward                 phc/env/tasks/humanoid_im.py:1543-1574
  compute_humanoid_im_reset                phc/env/tasks/humanoid_im.py:1600-1628
  discount_values                          phc/learning/common_agent.py:493-505
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import PULSE_IM_RESET, PULSE_IM_REWARD, PULSE_IM_SELF_OBS, PULSE_IM_TASK_OBS, AmpObsArgs, ImStepArgs, RewardSpecs
from ._marshal import Filler, check as _dev, launch as _launch, mask_u8, ptr as _ptr, rows2d, select_envs, step_outputs

DEFAULT_REWARD_SPECS = {"k_pos": 100.0, "k_rot": 10.0, "k_vel": 0.1, "k_ang_vel": 0.1,
                        "w_pos": 0.5, "w_rot": 0.3, "w_vel": 0.1, "w_ang_vel": 0.1}


def _c(t, name, dtype=torch.float32):
    t = _dev(t, name, dtype)             # (a tensor that is not on the GPU is a ValueError in this module)
    return t if t.is_contiguous() else t.contiguous()


# --------------------------------------------------------------------------- #
# rotation algebra
# --------------------------------------------------------------------------- #
def _rows(t, width, name):
    if t.shape[-1] != width:
        raise ValueError(f"{name}: last dim must be {width}, got {tuple(t.shape)}")
    return t.numel() // width


def quat_mul(a, b):
    a, b = _c(a, "a"), _c(b, "b")
    if a.shape != b.shape:
        raise AssertionError("quat_mul: shape mismatch")  # the reference asserts equal shapes
    out = torch.empty_like(a)
    _launch("pulse_quat_mul", _ptr(a), _ptr(b), _ptr(out), _rows(a, 4, "a"))
    return out


def quat_conjugate(a):
    a = _c(a, "a")
    out = torch.empty_like(a)
    _launch("pulse_quat_conjugate", _ptr(a), _ptr(out), _rows(a, 4, "a"))
    return out


def my_quat_rotate(q, v):
    q, v = _c(q, "q"), _c(v, "v")
    m = _rows(q, 4, "q")
    if _rows(v, 3, "v") != m:
        raise ValueError("my_quat_rotate: q and v row counts differ")
    out = torch.empty_like(v)
    _launch("pulse_quat_rotate", _ptr(q), _ptr(v), _ptr(out), m)
    return out


def quat_to_angle_axis(q):
    q = _c(q, "q")
    m = _rows(q, 4, "q")
    angle = torch.empty(q.shape[:-1], dtype=torch.float32, device=q.device)
    axis = torch.empty(q.shape[:-1] + (3,), dtype=torch.float32, device=q.device)
    _launch("pulse_quat_to_angle_axis", _ptr(q), _ptr(angle), _ptr(axis), m)
    return angle, axis


def quat_to_exp_map(q):
    q = _c(q, "q")
    out = torch.empty(q.shape[:-1] + (3,), dtype=torch.float32, device=q.device)
    _launch("pulse_quat_to_exp_map", _ptr(q), _ptr(out), _rows(q, 4, "q"))
    return out


def quat_to_tan_norm(q):
    q = _c(q, "q")
    out = torch.empty(q.shape[:-1] + (6,), dtype=torch.float32, device=q.device)
    _launch("pulse_quat_to_tan_norm", _ptr(q), _ptr(out), _rows(q, 4, "q"))
    return out


def exp_map_to_quat(e):
    e = _c(e, "exp_map")
    out = torch.empty(e.shape[:-1] + (4,), dtype=torch.float32, device=e.device)
    _launch("pulse_exp_map_to_quat", _ptr(e), _ptr(out), _rows(e, 3, "exp_map"))
    return out


def slerp(q0, q1, t):
    q0, q1 = _c(q0, "q0"), _c(q1, "q1")
    m = _rows(q0, 4, "q0")
    t = _c(t, "t").reshape(-1)
    if q1.shape != q0.shape or t.numel() != m:
        raise ValueError("slerp: shape mismatch")
    out = torch.empty_like(q0)
    _launch("pulse_slerp", _ptr(q0), _ptr(q1), _ptr(t), _ptr(out), m)
    return out


def calc_heading(q):
    q = _c(q, "q")
    out = torch.empty(q.shape[:-1], dtype=torch.float32, device=q.device)
    _launch("pulse_calc_heading", _ptr(q), _ptr(out), _rows(q, 4, "q"))
    return out


def calc_heading_quat(q):
    q = _c(q, "q")
    out = torch.empty_like(q)
    _launch("pulse_calc_heading_quat", _ptr(q), _ptr(out), _rows(q, 4, "q"), 0)
    return out


def calc_heading_quat_inv(q):
    q = _c(q, "q")
    out = torch.empty_like(q)
    _launch("pulse_calc_heading_quat", _ptr(q), _ptr(out), _rows(q, 4, "q"), 1)
    return out


# --------------------------------------------------------------------------- #
# fused HumanoidIm post-physics step
# --------------------------------------------------------------------------- #
def _specs_struct(specs=None, power_coef=0.0005, power_reward=True):
    s = dict(DEFAULT_REWARD_SPECS)
    if specs:
        s.update(specs)
    return RewardSpecs(s["k_pos"], s["k_rot"], s["k_vel"], s["k_ang_vel"], s["w_pos"], s["w_rot"], s["w_vel"],
                       s["w_ang_vel"], float(power_coef), 1 if power_reward else 0)


def pack_rb(body_pos, body_rot, body_vel, body_ang_vel):
    """Return an (N, J, 13) AoS tensor for the four body tensors.

    When they are the reference-style VIEWS of one Isaac rigid-body buffer
    (phc/env/tasks/humanoid.py:219-222) the buffer itself is returned (zero copy);
    otherwise (gathered copies) the records are re-packed.
    """
    p = _dev(body_pos, "body_pos")
    n, j = p.shape[0], p.shape[1]
    ts = (body_pos, body_rot, body_vel, body_ang_vel)
    offs = (0, 3, 7, 10)
    try:
        same = all(t.untyped_storage().data_ptr() == p.untyped_storage().data_ptr() for t in ts)
    except Exception:
        same = False
    if same and all(t.stride()[-1] == 1 and t.stride()[-2] == 13 for t in ts):
        base_off = p.storage_offset()
        if all(t.storage_offset() - base_off == o for t, o in zip(ts, offs)) and all(t.stride() == p.stride() for t in ts):
            return torch.as_strided(p, (n, j, 13), (p.stride()[0], 13, 1), base_off)
    return torch.cat([_dev(t, "body tensor") for t in ts], dim=-1).contiguous()


# PULSE_IM_DEBUG_POISON_LDS (include/pulse_hip.h): debug builds of a run can ask the fused step to pre-fill its LDS with NaN
_IM_DEBUG_BITS = 0x80000000 if os.environ.get("PULSE_IM_DEBUG_POISON_LDS") == "1" else 0


def _launch_sig(o):
    """Cheap identity of a launch's arguments: device pointers of tensors, values of scalars / id lists, recursively through dicts.  Two calls
    with equal signatures launch the same kernel on the same buffers (a buffer's layout is taken to be fixed by its address and element count)."""
    if o is None:
        return 0
    if isinstance(o, torch.Tensor):
        # (the caching allocator may hand a freed address to a tensor of another size; a view of the same storage may have another dtype / stride)
        return (o.data_ptr(), o.numel(), o.dtype, o.stride())
    if isinstance(o, dict):
        return tuple((k, _launch_sig(v)) for k, v in o.items())
    if isinstance(o, (list, tuple)):
        return tuple(_launch_sig(v) for v in o)
    sig = getattr(o, "launch_signature", None)
    return sig() if sig is not None else o


def _obs_copy_fields(obs_copy, n, cols, dev):
    """(pointer, row stride) of im_step's second observation destination; (None, 0) without one."""
    if obs_copy is None:
        return None, 0
    if (obs_copy.dtype != torch.float32 or obs_copy.device != dev or obs_copy.dim() != 2 or obs_copy.stride(1) != 1 or obs_copy.shape[0] != n or
            obs_copy.shape[1] < cols or obs_copy.stride(0) < cols):
        raise ValueError(f"obs_copy must be a ({n}, >= {cols}) float32 view on {dev} with unit inner stride")
    return obs_copy.data_ptr(), obs_copy.stride(0)


def im_step(rb, *, what, ref_now=None, ref_next=None, time_steps=1, dof_force=None, dof_vel=None,
            progress=None, pass_time=None, cycle_counter=None, track_ids=None, reset_ids=None, term_dist=None,
            reset_use_mean=False, full_body_reward=True, obs_version=6, local_root_obs=True,
            root_height_obs=True, specs=None, power_coef=0.0005, power_reward=True,
            env_ids=None, env_mask=None, obs=None, obs_cols=None, rew=None, rew_raw=None, reset=None,
            terminate=None, clock=None, motion=None, upright=True, enable_early_termination=True, self_obs_version=1,
            force_sensor=None, dof_pos=None, ref_next_dof_pos=None, smpl_params=None, limb_weights=None, recovery_counter=None, cache=None,
            zero_out_far=None, occl_bits=None, occl_reset=False, obs_copy=None):
    """``obs_copy``: a second (N, >= obs_cols) float32 view (any row pitch, e.g. an experience-buffer slot) that receives the same observation rows
    as ``obs``; NOT part of a cached launch's signature -- the pointer is patched into the cached struct on every call.
    ``occl_bits``: (N,) int32, bit j = tracked body j of the env is occluded (occl_training, humanoid_im.py:778-784, 827-831); ``occl_reset``:
    occluded reset bodies never count as fallen (:1178-1183).
    ``zero_out_far``: dict(point_goal (N,) float32 read by the reward stage / written by the task-observation stage, close_distance,
    far_distance) -- the far-masking branch of _compute_task_obs / _compute_reward (humanoid_im.py:763-777, 814-826, 870-887).
    ``cache``: a dict owned by a caller that launches the same step on the same buffers over and over (the env's post-physics step): the
    filled argument struct is kept in it and re-launched as long as the arguments' signature (_launch_sig) does not change -- the struct takes
    ~40 tensor checks to build, a third of the rollout's host time.
    ``clock``: dict(progress_rw, inc, dt, start_times, start_offsets, motion_len, cycle_motion, max_episode_length,
    pass_time_out) -- the episode clock advanced / evaluated in-kernel.  ``motion``: dict(lib, ids, offset, traj_dt, track_rb,
    track_dof_pos, track_dof_vel) -- the reference evaluated in-kernel from a MotionLib instead of ref_now / ref_next.
    Low-level entry: one launch of pulse_im_step.  ``rb`` is (N, J, 13) with unit inner strides
    (the env stride may be larger).  ref_* are dicts with keys pos/rot/vel/ang.  Outputs that are
    not supplied are allocated.  Returns dict(obs, rew, rew_raw, reset, terminate)."""
    kw = {k: v for k, v in locals().items() if k not in ("rb", "cache", "obs_copy")}       # first statement: exactly the other parameters
    sig = _im_step_signature(rb, **kw) if cache is not None else None
    if cache is not None and cache.get("sig") == sig:
        a, out, fill = cache["args"], cache["out"], None
    else:
        a, out, fill, owned = _im_step_fill(rb, **kw)
    if "obs" in out:
        a.obs_copy, a.obs_copy_stride = _obs_copy_fields(obs_copy, a.num_envs, a.obs_cols, rb.device)
    elif obs_copy is not None:
        raise ValueError("obs_copy without an observation stage")
    _launch("pulse_im_step", ctypes.byref(a))
    if cache is not None and fill is not None:
        cache.clear()
        if owned and not fill.copied:
            cache.update(sig=sig, args=a, keep=fill.keep, out=out)
    return out


def _im_step_signature(rb, **kw):
    """The identity of an im_step launch for its cache: everything the struct-filling body receives -- a keyword added to im_step is part
    of it without being listed anywhere -- and the module's debug bits as they are now."""
    return _launch_sig((rb, kw, _IM_DEBUG_BITS))


def _im_step_fill(rb, *, what, ref_now, ref_next, time_steps, dof_force, dof_vel, progress, pass_time, cycle_counter, track_ids, reset_ids, term_dist,
                  reset_use_mean, full_body_reward, obs_version, local_root_obs, root_height_obs, specs, power_coef, power_reward, env_ids, env_mask,
                  obs, obs_cols, rew, rew_raw, reset, terminate, clock, motion, upright, enable_early_termination, self_obs_version, force_sensor,
                  dof_pos, ref_next_dof_pos, smpl_params, limb_weights, recovery_counter, zero_out_far, occl_bits, occl_reset):
    """im_step's struct-filling body -> (pulse_im_step_args without its obs_copy fields, the outputs dict, the Filler that keeps the
    struct's tensors alive, whether every output is the caller's).  Only a launch whose outputs are all caller-owned may be replayed: an
    output this wrapper allocates would be a new buffer on every call."""
    lib = _lib.load()
    owned = ((obs is not None or not what & (PULSE_IM_SELF_OBS | PULSE_IM_TASK_OBS)) and
             ((rew is not None and rew_raw is not None) or not what & PULSE_IM_REWARD) and
             ((reset is not None and terminate is not None) or not what & PULSE_IM_RESET))
    rb = _dev(rb, "rb")
    hist = 1
    if self_obs_version == 2:                      # (N, H, J, 13) history, oldest first (compute_humanoid_observations_smpl_max_v2)
        if rb.dim() != 4 or not rb[0].is_contiguous():
            raise ValueError("self_obs_version 2 takes rb as (N, H, J, 13) with contiguous per-env histories")
        hist = rb.shape[1]
        rb = rb.view(rb.shape[0], hist * rb.shape[2], 13) if rb.is_contiguous() else rb
    if rb.dim() == 4:
        n, j = rb.shape[0], rb.shape[2]
        rb_stride = rb.stride()[0]
    else:
        if rb.dim() != 3 or rb.shape[-1] != 13 or rb.stride()[-1] != 1 or rb.stride()[-2] != 13:
            raise ValueError("rb must be (N, J, 13) with contiguous body records")
        n, j = rb.shape[0], rb.shape[1] // hist
        rb_stride = rb.stride()[0]
    dev = rb.device
    a = ImStepArgs()
    P = Filler()
    P.keep.append(rb)
    a.rb, a.rb_env_stride, a.num_envs, a.num_bodies = rb.data_ptr(), rb_stride, n, j
    a.upright_start, a.enable_early_termination = int(bool(upright)), int(bool(enable_early_termination))
    a.self_obs_version, a.hist_steps = int(self_obs_version), hist
    fsw = 0
    if force_sensor is not None:
        a.force_sensor, a.force_sensor_width = P(force_sensor, "force_sensor"), force_sensor.shape[-1]
        fsw = force_sensor.shape[-1]
    for name, t in (("smpl_params", smpl_params), ("limb_weights", limb_weights)):     # rows appended to the self observation
        if t is not None:
            _dev(t, name)
            if t.dim() != 2 or t.shape[0] != n or t.stride(1) != 1:
                raise ValueError(f"{name}: (num_envs, width) with contiguous rows expected")
            P.keep.append(t)
            setattr(a, name, t.data_ptr()); setattr(a, name + "_width", t.shape[1]); setattr(a, name + "_stride", t.stride(0))
            fsw += t.shape[1]
    if recovery_counter is not None:
        a.recovery_counter = P(recovery_counter, "recovery_counter", torch.int32)
    if occl_bits is not None:
        if occl_bits.shape != (n,) or occl_bits.dtype != torch.int32:
            raise ValueError("occl_bits: (num_envs,) int32 expected")
        a.occl_bits, a.occl_reset = P(occl_bits, "occl_bits", torch.int32), int(bool(occl_reset))
    if zero_out_far is not None:
        pg = zero_out_far["point_goal"]
        if pg.shape != (n,) or not pg.is_contiguous():
            raise ValueError("zero_out_far.point_goal: contiguous (num_envs,) float32 expected")
        a.zero_out_far, a.point_goal = 1, P(pg, "zero_out_far.point_goal")
        a.close_distance, a.far_distance = float(zero_out_far.get("close_distance", 0.25)), float(zero_out_far.get("far_distance", 3.0))
    a.dof_pos, a.ref_next_dof_pos = P(dof_pos, "dof_pos"), P(ref_next_dof_pos, "ref_next_dof_pos")
    if dof_pos is not None and dof_force is None:
        a.num_dof = dof_pos.shape[-1]
    select_envs(a, P, env_ids, env_mask)
    if ref_now is not None:
        a.ref_now_pos, a.ref_now_rot = P(ref_now["pos"], "ref_now.pos"), P(ref_now["rot"], "ref_now.rot")
        a.ref_now_vel, a.ref_now_ang = P(ref_now["vel"], "ref_now.vel"), P(ref_now["ang"], "ref_now.ang")
    if ref_next is not None:
        a.ref_next_pos, a.ref_next_vel = P(ref_next["pos"], "ref_next.pos"), P(ref_next["vel"], "ref_next.vel")
        a.ref_next_rot, a.ref_next_ang = P(ref_next.get("rot"), "ref_next.rot"), P(ref_next.get("ang"), "ref_next.ang")
    a.time_steps = time_steps
    a.dof_force, a.dof_vel = P(dof_force, "dof_force"), P(dof_vel, "dof_vel")
    if dof_force is not None:
        a.num_dof = dof_force.shape[-1]
    a.progress = P(progress, "progress", torch.int64)
    if pass_time is not None:
        a.pass_time = P(mask_u8(pass_time), "pass_time", torch.uint8)
    a.cycle_counter = P(cycle_counter, "cycle_counter", torch.int64)
    if track_ids is not None:
        a.track_ids, a.num_track = P.ids32(track_ids, "track_ids", dev)
    if reset_ids is not None:
        a.reset_ids, a.num_reset = P.ids32(reset_ids, "reset_ids", dev)
    a.term_dist = P(term_dist, "term_dist")
    a.reset_use_mean, a.full_body_reward = int(reset_use_mean), int(full_body_reward)
    a.what, a.obs_version = what | _IM_DEBUG_BITS, obs_version
    a.local_root_obs, a.root_height_obs = int(local_root_obs), int(root_height_obs)
    a.specs = _specs_struct(specs, power_coef, power_reward)

    out = {}
    if what & (PULSE_IM_SELF_OBS | PULSE_IM_TASK_OBS):
        sw = lib.pulse_self_obs_width_ex(j, int(root_height_obs), int(self_obs_version), hist, fsw)
        tw = lib.pulse_task_obs_width(obs_version, a.num_track, time_steps) if what & PULSE_IM_TASK_OBS else 0
        width = sw + tw
        if obs is None:
            obs = torch.empty(n, width if obs_cols is None else obs_cols, dtype=torch.float32, device=dev)
        _dev(obs, "obs")
        if obs.stride()[-1] != 1:
            raise ValueError("obs rows must be contiguous")
        a.obs, a.obs_stride = obs.data_ptr(), obs.stride()[0]
        a.obs_cols = width if obs_cols is None else obs_cols
        out["obs"] = obs
    step_outputs(a, P, out, n, dev, reward=what & PULSE_IM_REWARD, resets=what & PULSE_IM_RESET, raw_width=5 if power_reward else 4,
                 rew=rew, rew_raw=rew_raw, reset=reset, terminate=terminate)
    if clock is not None:
        a.progress_rw, a.progress_inc = P(clock.get("progress_rw"), "clock.progress_rw", torch.int64), int(clock.get("inc", 0))
        a.clock_dt = float(clock.get("dt", 0.0))
        a.clock_start_times, a.clock_start_offsets = P(clock.get("start_times"), "clock.start_times"), P(clock.get("start_offsets"), "clock.start_offsets")
        a.clock_motion_len = P(clock.get("motion_len"), "clock.motion_len")
        a.cycle_motion, a.max_episode_length = int(bool(clock.get("cycle_motion", False))), int(clock.get("max_episode_length", 0))
        pto = clock.get("pass_time_out")
        if pto is not None:
            a.pass_time_out = P(mask_u8(pto), "clock.pass_time_out", torch.uint8)
    if motion is not None:
        a.use_motion = 1
        motion["lib"].fill_tables(a.motion)
        a.motion_ids, a.motion_offset = P(motion["ids"], "motion.ids", torch.int64), P(motion.get("offset"), "motion.offset")
        a.traj_dt = float(motion.get("traj_dt", 0.0))
        trb = motion.get("track_rb")
        if trb is not None:
            a.track_rb, a.track_rb_stride = P(trb, "motion.track_rb"), trb.stride(0)
        a.track_dof_pos, a.track_dof_vel = P(motion.get("track_dof_pos"), "motion.track_dof_pos"), P(motion.get("track_dof_vel"), "motion.track_dof_vel")
    return a, out, P, owned


def compute_humanoid_observations_smpl_max(body_pos, body_rot, body_vel, body_ang_vel, smpl_params=None,
                                           limb_weight_params=None, local_root_obs=True, root_height_obs=True,
                                           upright=True, has_smpl_params=False, has_limb_weight_params=False):
    """phc/env/tasks/humanoid.py:1675-1731 (shape / limb-weight rows appended when has_* is set, :1724-1728); upright=False applies
    remove_base_rot (:1616-1620)."""
    rb = pack_rb(body_pos, body_rot, body_vel, body_ang_vel)
    return im_step(rb, what=PULSE_IM_SELF_OBS, local_root_obs=local_root_obs, root_height_obs=root_height_obs, upright=upright,
                   smpl_params=smpl_params if has_smpl_params else None, limb_weights=limb_weight_params if has_limb_weight_params else None)["obs"]


def compute_humanoid_observations_smpl_max_v2(body_pos, body_rot, body_vel, body_ang_vel, smpl_params=None, limb_weight_params=None,
                                              local_root_obs=True, root_height_obs=True, upright=True, has_smpl_params=False,
                                              has_limb_weight_params=False, time_steps=1):
    """phc/env/tasks/humanoid.py:1734-1786: (B, T, J, .) history in the heading frame of the newest root."""
    if has_smpl_params or has_limb_weight_params or not local_root_obs:
        raise NotImplementedError("the reference itself raises for these options (humanoid.py:1766-1783)")
    rb = torch.cat([body_pos, body_rot, body_vel, body_ang_vel], dim=-1).contiguous()
    return im_step(rb, what=PULSE_IM_SELF_OBS, local_root_obs=True, root_height_obs=root_height_obs, upright=upright, self_obs_version=2)["obs"]


def compute_humanoid_observations_smpl_max_v3(body_pos, body_rot, body_vel, body_ang_vel, force_sensor_readings, smpl_params=None,
                                              limb_weight_params=None, local_root_obs=True, root_height_obs=True, upright=True,
                                              has_smpl_params=False, has_limb_weight_params=False):
    """phc/env/tasks/humanoid.py:1789-1849: _smpl_max + the force-sensor readings (+ shape / limb-weight rows, :1843-1847)."""
    rb = pack_rb(body_pos, body_rot, body_vel, body_ang_vel)
    return im_step(rb, what=PULSE_IM_SELF_OBS, local_root_obs=local_root_obs, root_height_obs=root_height_obs, upright=upright,
                   self_obs_version=3, force_sensor=force_sensor_readings,
                   smpl_params=smpl_params if has_smpl_params else None, limb_weights=limb_weight_params if has_limb_weight_params else None)["obs"]


def remove_base_rot(quat):
    """phc/env/tasks/humanoid.py:1616-1620."""
    base = torch.tensor([[-0.5, -0.5, -0.5, 0.5]], dtype=torch.float32, device=quat.device).repeat(quat.shape[0], 1)
    return quat_mul(quat, base)


def compute_imitation_observations_v6(root_pos, root_rot, body_pos, body_rot, body_vel, body_ang_vel,
                                      ref_body_pos, ref_body_rot, ref_body_vel, ref_body_ang_vel, time_steps, upright=True):
    """phc/env/tasks/humanoid_im.py:1328-1378.  body_* are the tracked subset (B, Jt, .); the root
    is passed separately exactly as in the reference."""
    return _task_obs(6, root_pos, root_rot, body_pos, body_rot, body_vel, body_ang_vel,
                     ref_body_pos, ref_body_rot, ref_body_vel, ref_body_ang_vel, time_steps, upright)


def compute_imitation_observations(root_pos, root_rot, body_pos, body_rot, body_vel, body_ang_vel,
                                   ref_body_pos, ref_body_rot, ref_body_vel, ref_body_ang_vel, time_steps, upright=True):
    """obs_v 1, phc/env/tasks/humanoid_im.py:1222-1256."""
    return _task_obs(1, root_pos, root_rot, body_pos, body_rot, body_vel, body_ang_vel, ref_body_pos, ref_body_rot, ref_body_vel,
                     ref_body_ang_vel, time_steps, upright)


def compute_imitation_observations_v2(root_pos, root_rot, body_pos, body_rot, body_vel, body_ang_vel, dof_pos, ref_body_pos, ref_body_rot,
                                      ref_body_vel, ref_body_ang_vel, ref_dof_pos, time_steps, upright=True):
    """obs_v 2, phc/env/tasks/humanoid_im.py:1259-1297: v1 + dof differences (dof_pos / ref_dof_pos: (B, Jt - 1, 3) subsets)."""
    return _task_obs(2, root_pos, root_rot, body_pos, body_rot, body_vel, body_ang_vel, ref_body_pos, ref_body_rot, ref_body_vel,
                     ref_body_ang_vel, time_steps, upright, dof_pos=dof_pos, ref_dof_pos=ref_dof_pos)


def compute_imitation_observations_v3(root_pos, root_rot, body_pos, body_rot, body_vel, body_ang_vel,
                                      ref_body_pos, ref_body_rot, ref_body_vel, ref_body_ang_vel, time_steps, upright=True):
    """obs_v 3, phc/env/tasks/humanoid_im.py:1300-1325."""
    return _task_obs(3, root_pos, root_rot, body_pos, body_rot, body_vel, body_ang_vel, ref_body_pos, ref_body_rot, ref_body_vel,
                     ref_body_ang_vel, time_steps, upright)


def compute_imitation_observations_v8(root_pos, root_rot, body_pos, body_rot, body_vel, body_ang_vel,
                                      ref_body_pos, ref_body_rot, ref_body_vel, ref_body_ang_vel, time_steps, upright=True):
    """obs_v 8, phc/env/tasks/humanoid_im.py:1415-1481 (time_steps 1)."""
    return _task_obs(8, root_pos, root_rot, body_pos, body_rot, body_vel, body_ang_vel, ref_body_pos, ref_body_rot, ref_body_vel,
                     ref_body_ang_vel, time_steps, upright)


def compute_imitation_observations_v9(root_pos, root_rot, body_pos, body_rot, body_vel, body_ang_vel,
                                      ref_body_pos, ref_body_rot, ref_root_vel, ref_root_ang_vel, time_steps, upright=True):
    """obs_v 9, phc/env/tasks/humanoid_im.py:1484-1540: the reference passes only the ROOT reference velocities."""
    b, jt = body_pos.shape[0], body_pos.shape[1]
    rv = torch.zeros(b * time_steps, jt, 3, dtype=torch.float32, device=body_pos.device)
    ra = torch.zeros_like(rv)
    rv[:, 0], ra[:, 0] = ref_root_vel.reshape(-1, 3), ref_root_ang_vel.reshape(-1, 3)
    return _task_obs(9, root_pos, root_rot, body_pos, body_rot, body_vel, body_ang_vel, ref_body_pos, ref_body_rot, rv, ra, time_steps, upright)


def compute_imitation_observations_v7(root_pos, root_rot, body_pos, body_vel, ref_body_pos, ref_body_vel, time_steps, upright=True):
    """phc/env/tasks/humanoid_im.py:1381-1413."""
    z4 = torch.zeros(body_pos.shape[:-1] + (4,), dtype=torch.float32, device=body_pos.device)
    z4[..., 3] = 1.0
    z3 = torch.zeros_like(body_pos)
    return _task_obs(7, root_pos, root_rot, body_pos, z4, body_vel, z3, ref_body_pos, None, ref_body_vel, None, time_steps, upright)


def _task_obs(version, root_pos, root_rot, bp, br, bv, ba, rp, rr, rv, ra, time_steps, upright=True, dof_pos=None, ref_dof_pos=None):
    # The kernel indexes bodies through a track list and reads the root from body 0, so build
    # a (B, 1 + Jt, 13) record array: slot 0 = root, slots 1.. = the tracked subset.
    b, jt = bp.shape[0], bp.shape[1]
    dev = bp.device
    root = torch.zeros(b, 1, 13, dtype=torch.float32, device=dev)
    root[:, 0, 0:3] = root_pos
    root[:, 0, 3:7] = root_rot
    rb = torch.cat([root, torch.cat([bp, br, bv, ba], dim=-1)], dim=1).contiguous()
    j = 1 + jt

    def pad(x, w):  # (B*T, Jt, w) -> (B*T, 1+Jt, w)
        x = x.reshape(b * time_steps, jt, w)
        return torch.cat([torch.zeros(b * time_steps, 1, w, dtype=torch.float32, device=dev), x], dim=1).contiguous()

    ref_next = {"pos": pad(rp, 3), "vel": pad(rv, 3)}
    if version != 7:
        ref_next["rot"], ref_next["ang"] = pad(rr, 4), pad(ra, 3)
    lib = _lib.load()
    sw = lib.pulse_self_obs_width(j, 1)
    tw = lib.pulse_task_obs_width(version, jt, time_steps)
    full = torch.empty(b, sw + tw, dtype=torch.float32, device=dev)
    kw = {}
    if version == 2:
        # joint (track id - 1) of the packed array = subset joint of tracked body i >= 1 (the root carries no dof)
        def dof_full(d):
            f = torch.zeros(b, 3 * (j - 1), dtype=torch.float32, device=dev)
            f[:, 3:] = d.reshape(b, -1)
            return f
        kw = {"dof_pos": dof_full(dof_pos), "ref_next_dof_pos": dof_full(ref_dof_pos)}
    im_step(rb, what=PULSE_IM_TASK_OBS, ref_next=ref_next, time_steps=time_steps, obs_version=version,
            track_ids=list(range(1, j)), obs=full, upright=upright, **kw)
    return full[:, sw:]


def compute_imitation_reward(root_pos, root_rot, body_pos, body_rot, body_vel, body_ang_vel,
                             ref_body_pos, ref_body_rot, ref_body_vel, ref_body_ang_vel, rwd_specs):
    """phc/env/tasks/humanoid_im.py:1543-1574 -> (reward (N,), reward_raw (N,4))."""
    rb = pack_rb(body_pos, body_rot, body_vel, body_ang_vel)
    n = rb.shape[0]
    dev = rb.device
    ref = {"pos": ref_body_pos, "rot": ref_body_rot, "vel": ref_body_vel, "ang": ref_body_ang_vel}
    out = im_step(rb, what=PULSE_IM_REWARD, ref_now=ref, specs=rwd_specs, power_reward=False,
                  progress=torch.zeros(n, dtype=torch.int64, device=dev))
    return out["rew"], out["rew_raw"]


def compute_humanoid_im_reset(reset_buf, progress_buf, contact_buf, contact_body_ids, rigid_body_pos, ref_body_pos,
                              pass_time, enable_early_termination, termination_distance, disableCollision, use_mean):
    """phc/env/tasks/humanoid_im.py:1600-1628.  rigid_body_pos / ref_body_pos are already restricted
    to the reset bodies (N, Jr, 3); termination_distance is (Jr,) or (1, Jr)."""
    n, jr = rigid_body_pos.shape[0], rigid_body_pos.shape[1]
    dev = rigid_body_pos.device
    if (not enable_early_termination) or disableCollision:
        term = torch.zeros_like(reset_buf)
        return torch.where(pass_time, torch.ones_like(reset_buf), term), term
    rb = torch.zeros(n, jr, 13, dtype=torch.float32, device=dev)
    rb[..., 0:3] = rigid_body_pos
    rb[..., 6] = 1.0
    z3 = torch.zeros(n, jr, 3, dtype=torch.float32, device=dev)
    z4 = torch.zeros(n, jr, 4, dtype=torch.float32, device=dev)
    ref = {"pos": ref_body_pos, "rot": z4, "vel": z3, "ang": z3}
    td = termination_distance.reshape(-1).to(torch.float32)
    if td.numel() == 1:
        td = td.expand(jr)
    out = im_step(rb, what=PULSE_IM_RESET, ref_now=ref, progress=progress_buf, pass_time=pass_time,
                  reset_ids=list(range(jr)), term_dist=td.contiguous(), reset_use_mean=use_mean)
    return out["reset"], out["terminate"]


# --------------------------------------------------------------------------- #
# evaluation metrics (IMAmpAgent.eval): one launch of pulse_im_eval_accum per control step
# --------------------------------------------------------------------------- #
EVAL_ACCUM_COLUMNS = ("mpjpe_g", "mpjpe_l", "mpjpe_pa", "vel_dist", "accel_dist", "frames", "vel_frames", "accel_frames")


def im_eval_state(num_envs, num_bodies, device):
    """The per-env state of an evaluation sweep: the two-step position ring (N, 2, 2, J, 3) float32 and the accumulator rows (N, 8)
    float64 (EVAL_ACCUM_COLUMNS: five sums in mm, three frame counts)."""
    return (torch.zeros(num_envs, 2, 2, num_bodies, 3, dtype=torch.float32, device=device),
            torch.zeros(num_envs, 8, dtype=torch.float64, device=device))


def im_eval_accum(rb, ref_pos, num_steps, step, ring, accum, *, env_mask=None):
    """Add control step ``step`` (0-based index inside the evaluation batch) to the per-env metric sums (include/pulse_hip.h 2b'').
    ``rb`` (N, J, 13) simulated records and ``ref_pos`` (N, J, 3) reference positions may be row-strided views (any env pitch, bodies
    contiguous); ``num_steps`` (N) int32; ``accum`` (N, 8) float64, row-strided allowed; ``ring`` contiguous (N, 2, 2, J, 3).
    ``env_mask`` (N) bool / uint8: envs with 0 are left alone."""
    rb, ref_pos, ring = _dev(rb, "rb"), _dev(ref_pos, "ref_pos"), _dev(ring, "ring")
    accum, num_steps = _dev(accum, "accum", torch.float64), _dev(num_steps, "num_steps", torch.int32)
    if rb.dim() != 3 or rb.shape[2] != 13:
        raise ValueError(f"rb: expected (N, J, 13), got {tuple(rb.shape)}")
    n, j = rb.shape[0], rb.shape[1]
    if tuple(ref_pos.shape) != (n, j, 3):
        raise ValueError(f"ref_pos: expected shape {(n, j, 3)}, got {tuple(ref_pos.shape)}")
    if (j > 1 and rb.stride(1) != 13) or rb.stride(2) != 1:
        raise ValueError("rb: the (J, 13) records of an env must be contiguous (only the env pitch may be larger)")
    if (j > 1 and ref_pos.stride(1) != 3) or ref_pos.stride(2) != 1:
        raise ValueError("ref_pos: the (J, 3) positions of an env must be contiguous (only the env pitch may be larger)")
    if tuple(ring.shape) != (n, 2, 2, j, 3) or not ring.is_contiguous():
        raise ValueError(f"ring: contiguous {(n, 2, 2, j, 3)} expected, got {tuple(ring.shape)}")
    if tuple(accum.shape) != (n, 8) or accum.stride(1) != 1:
        raise ValueError(f"accum: expected shape {(n, 8)} with contiguous rows, got {tuple(accum.shape)}")
    if tuple(num_steps.shape) != (n,) or not num_steps.is_contiguous():
        raise ValueError(f"num_steps: contiguous {(n,)} expected")
    a = _lib.ImEvalArgs()
    a.rb, a.rb_env_stride = rb.data_ptr(), rb.stride(0) if n > 1 else 13 * j
    a.ref_pos, a.ref_env_stride = ref_pos.data_ptr(), ref_pos.stride(0) if n > 1 else 3 * j
    a.num_envs, a.num_bodies, a.num_steps, a.step = n, j, num_steps.data_ptr(), int(step)
    if env_mask is not None:
        m = _dev(env_mask, "env_mask", torch.uint8)
        if tuple(m.shape) != (n,) or not m.is_contiguous():
            raise ValueError(f"env_mask: contiguous device {(n,)} bool / uint8 expected")
        a.env_mask = m.data_ptr()
    a.ring, a.accum, a.accum_stride = ring.data_ptr(), accum.data_ptr(), accum.stride(0) if n > 1 else 8
    _launch("pulse_im_eval_accum", ctypes.byref(a))
    return accum


# --------------------------------------------------------------------------- #
# downstream tasks (speed / reach / strike): one launch of pulse_task_step
# --------------------------------------------------------------------------- #
def task_step(task, rb, *, what, prev_root_pos=None, dt=1.0 / 30.0, tar_speed=None, tar_pos=None, reach_body_id=0, tar_states=None,
              tar_contact_forces=None, strike_body_ids=None, contact_forces=None, contact_body_ids=None, termination_heights=None,
              progress=None, max_episode_length=300.0, enable_early_termination=True, dof_force=None, dof_vel=None, power_coef=0.0005,
              power_reward=False, obs=None, obs_offset=0, rew=None, rew_raw=None, reset=None, terminate=None, env_ids=None, env_mask=None):
    """``task``: 'speed' | 'reach' | 'strike'.  ``rb`` (N, J, 13).  Returns dict(obs, rew, rew_raw, reset, terminate) of what was asked."""
    from ._lib import TASK_OBS, TASK_REACH, TASK_RESET, TASK_REWARD, TASK_SPEED, TASK_STRIKE, TaskStepArgs
    lib = _lib.load()
    rb = _dev(rb, "rb")
    n, j = rb.shape[0], rb.shape[1]
    dev = rb.device
    a = TaskStepArgs()
    P = Filler()
    a.task = {"speed": TASK_SPEED, "reach": TASK_REACH, "strike": TASK_STRIKE}[task]
    a.what, a.num_envs = what, n
    a.rb, a.rb_env_stride, a.num_bodies = rb.data_ptr(), rb.stride()[0], j
    select_envs(a, P, env_ids, env_mask)
    a.prev_root_pos, a.dt = P(prev_root_pos, "prev_root_pos"), float(dt)
    a.tar_speed, a.tar_pos, a.reach_body_id = P(tar_speed, "tar_speed"), P(tar_pos, "tar_pos"), int(reach_body_id)
    a.tar_states, a.tar_contact_forces = P(tar_states, "tar_states"), P(tar_contact_forces, "tar_contact_forces")
    if strike_body_ids is not None:
        a.strike_body_ids, a.num_strike = P.ids32(strike_body_ids, "strike_body_ids", dev)
    if contact_body_ids is not None:
        a.contact_body_ids, a.num_contact_ids = P.ids32(contact_body_ids, "contact_body_ids", dev)
    a.contact_forces, a.termination_heights = P(contact_forces, "contact_forces"), P(termination_heights, "termination_heights")
    a.progress, a.max_episode_length = P(progress, "progress", torch.int64), float(max_episode_length)
    a.enable_early_termination = int(bool(enable_early_termination))
    a.dof_force, a.dof_vel = P(dof_force, "dof_force"), P(dof_vel, "dof_vel")
    a.num_dof = dof_force.shape[-1] if dof_force is not None else 0
    a.power_coef, a.power_reward = float(power_coef), int(bool(power_reward))
    out = {}
    if what & TASK_OBS:
        w = lib.pulse_task_obs_size(a.task)
        if obs is None:
            obs = torch.empty(n, obs_offset + w, dtype=torch.float32, device=dev)
        _dev(obs, "obs")
        a.obs, a.obs_stride, a.obs_offset = obs.data_ptr(), obs.stride()[0], int(obs_offset)
        out["obs"] = obs
    if what & TASK_REWARD:                     # (a caller's rew_raw sets the raw-reward width the kernel writes)
        a.rew_raw_width = rew_raw.shape[-1] if rew_raw is not None else (2 if power_reward else 1)
    step_outputs(a, P, out, n, dev, reward=what & TASK_REWARD, resets=what & TASK_RESET, raw_width=a.rew_raw_width,
                 rew=rew, rew_raw=rew_raw, reset=reset, terminate=terminate)
    _launch("pulse_task_step", ctypes.byref(a))
    return out


# --------------------------------------------------------------------------- #
# AMP observation
# --------------------------------------------------------------------------- #
def amp_obs_width(num_joints, num_key_bodies, root_height_obs=True, *, version=1, num_shape=0, num_limb=0):
    """_num_amp_obs_per_step of the SMPL humanoids (humanoid_amp.py:299-314)."""
    if version not in (1, 2):
        raise ValueError(f"amp_obs_width: version must be 1 or 2, got {version!r}")
    return _lib.load().pulse_amp_obs_width_v(num_joints, num_key_bodies, int(root_height_obs), int(version), int(num_shape), int(num_limb))


def _amp_variant(a, P, fn, rows, dev, *, key_body_ids, joint_ids, all_joints, local_root_obs, root_height_obs, upright, version, shape_params,
                 limb_weights):
    """The fields pulse_amp_obs_args and pulse_amp_hist_args share: the key-body / joint selection (``all_joints`` without one), the root
    options, upright_start, version, the optional shape / limb rows (``rows`` of them).  -> the frame width they give."""
    if version not in (1, 2):
        raise ValueError(f"{fn}: version must be 1 or 2, got {version!r}")
    a.key_body_ids, a.num_key_bodies = P.ids32(key_body_ids, "key_body_ids", dev)
    a.num_joints = all_joints
    if joint_ids is not None:
        a.joint_ids, a.num_joints = P.ids32(joint_ids, "joint_ids", dev)
    a.local_root_obs, a.root_height_obs = int(local_root_obs), int(root_height_obs)
    a.upright_start, a.version = int(bool(upright)), int(version)
    for name, t in (("shape_params", shape_params), ("limb_weights", limb_weights)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != rows:
            raise TypeError(f"{fn}: {name} must be a ({rows}, k) float32 tensor on {dev} with unit column stride")
        P.keep.append(t)
        if name == "shape_params":
            a.shape_params, a.shape_stride, a.num_shape = t.data_ptr(), t.stride(0), t.shape[1]
        else:
            a.limb_weights, a.limb_stride, a.num_limb = t.data_ptr(), t.stride(0), t.shape[1]
    return _lib.load().pulse_amp_obs_width_v(a.num_joints, a.num_key_bodies, a.root_height_obs, a.version, a.num_shape, a.num_limb)


def build_amp_observations_smpl(rb, dof_pos, dof_vel, key_body_ids, *, joint_ids=None, zero_joints=(), local_root_obs=True,
                                root_height_obs=True, out=None, env_ids=None, env_mask=None, hist_steps=0, window_out=None,
                                upright=True, version=1, shape_params=None, limb_weights=None):
    """phc/env/tasks/humanoid_amp.py:925-969 (``version`` 2: :973-1017) on the (N, bodies, 13) rigid-body records (root = body 0) and the
    (N, num_dof) dof tensors.  ``joint_ids`` = dof_subset expressed in joints; ``zero_joints`` = joints whose dofs
    read as zero (:636-639); ``upright`` False: remove_base_rot first (:929-930); ``shape_params`` (N, k) / ``limb_weights`` (N, k) rows are
    appended (has_shape_obs_disc / has_limb_weight_obs, :963-966; pass the truncated view ``humanoid_shapes[:, :-6]``).
    Writes the first W columns of ``out`` rows (any row pitch) and returns ``out``."""
    rb = _dev(rb, "rb")
    n = rb.shape[0]
    dev = rb.device
    a = AmpObsArgs()
    P = Filler()
    a.dof_pos, a.dof_vel, a.num_dof, a.num_envs = P(dof_pos, "dof_pos"), P(dof_vel, "dof_vel"), dof_pos.shape[-1], n
    w = _amp_variant(a, P, "build_amp_observations_smpl", n, dev, key_body_ids=key_body_ids, joint_ids=joint_ids, all_joints=dof_pos.shape[-1] // 3,
                     local_root_obs=local_root_obs, root_height_obs=root_height_obs, upright=upright, version=version, shape_params=shape_params,
                     limb_weights=limb_weights)
    if out is None:
        out = torch.empty(n, w, dtype=torch.float32, device=dev)
    a.rb, a.rb_env_stride = rb.data_ptr(), rb.stride()[0]
    select_envs(a, P, env_ids, env_mask)
    a.zero_joint_mask = sum(1 << int(j) for j in zero_joints)
    a.out, a.out_stride = out.data_ptr(), out.stride()[0]
    if hist_steps and hist_steps > 1:
        # ``out`` is slot 0 of the (N, hist_steps, W) history: shift + current frame (+ copy of the finished window) in this launch
        a.hist_steps = int(hist_steps)
        if window_out is not None:
            if window_out.dtype != torch.float32 or not window_out.is_cuda or window_out.stride(-1) != 1 or window_out.shape[0] != n:
                raise TypeError("build_amp_observations_smpl: window_out must be a float32 CUDA tensor with one row per env")
            a.window_out, a.window_stride = window_out.data_ptr(), window_out.stride(0)
    elif window_out is not None:
        raise ValueError("build_amp_observations_smpl: window_out goes with hist_steps > 1")
    _launch("pulse_amp_obs", ctypes.byref(a))
    return out


def amp_hist_init(motion_lib, motion_ids, start_times, dt, env_mask, hist, key_body_ids, *, joint_ids=None, local_root_obs=True, root_height_obs=True,
                  upright=True, version=1, shape_params=None, limb_weights=None):
    """_init_amp_obs_ref (humanoid_amp.py:531-563) for the masked envs: slots 1 .. S-1 of ``hist`` (N, S, W) := the AMP frames of each env's
    motion at start_times - dt * (k + 1), in one launch (pulse_amp_hist_init).  ``shape_params`` / ``limb_weights`` hold one row per MOTION
    (motion_bodies[:, :-6] / motion_limb_weights, :548-555); ``upright`` / ``version`` as build_amp_observations_smpl."""
    dev = hist.device
    if hist.dtype != torch.float32 or hist.dim() != 3 or hist.stride(2) != 1 or not hist.is_cuda:
        raise TypeError("amp_hist_init: hist must be a (N, S, W) float32 CUDA tensor")
    n, s_, w = hist.shape
    if motion_ids.numel() != n or start_times.numel() != n:
        raise ValueError("amp_hist_init: one motion id / start time per env")
    a = _lib.AmpHistArgs()
    P = Filler()
    if _amp_variant(a, P, "amp_hist_init", motion_lib.num_motions(), dev, key_body_ids=key_body_ids, joint_ids=joint_ids,
                    all_joints=motion_lib.num_bodies - 1, local_root_obs=local_root_obs, root_height_obs=root_height_obs, upright=upright,
                    version=version, shape_params=shape_params, limb_weights=limb_weights) != w:
        raise ValueError("amp_hist_init: the history's frame width does not match the joint / key-body selection, version and rows")
    motion_lib.fill_tables(a.tab)
    a.motion_ids, a.start_times, a.dt = P(motion_ids, "motion_ids", torch.int64), P(start_times, "start_times"), float(dt)
    a.num_envs, a.env_mask, a.hist_steps = n, P(mask_u8(env_mask), "env_mask", torch.uint8), s_
    a.hist, a.env_stride, a.step_stride = hist.data_ptr(), hist.stride(0), hist.stride(1)
    _launch("pulse_amp_hist_init", ctypes.byref(a))
    return hist


TASK_RESET_TRANSFORMS = {"none": _lib.TASK_RESET_NONE, "zero_xy": _lib.TASK_RESET_ZERO_XY, "remove_heading": _lib.TASK_RESET_REMOVE_HEADING,
                         "terrain": _lib.TASK_RESET_TERRAIN}


def task_ref_state_init(motion_lib, motion_ids, times, env_mask, rb, dof_pos, dof_vel, start_times, sampled_ids, *, clears=(), transform="none",
                        upright=True, new_root_xy=None, heightsamples=None, horizontal_scale=0.1, vertical_scale=0.005, center_points=None):
    """_reset_ref_state_init of the downstream tasks (humanoid_amp.py:447-488 with the task's _sample_ref_state) for the masked envs in one
    launch (pulse_task_ref_state_init): the clip ``motion_ids[e]`` blended at ``times[e]``, the task's root ``transform`` ('none' traj |
    'zero_xy' reach, strike | 'remove_heading' speed, takes ``upright`` | 'terrain', takes ``new_root_xy`` (N, 2), the int16 height field
    (None: terrainType 'plane'), its two scales and the (P, 2) centre grid) written into the simulator's tensors ``rb`` (N, J, 13),
    ``dof_pos`` / ``dof_vel`` (N, 3 (J - 1)) and into ``start_times`` (N,) float32 / ``sampled_ids`` (N,) int64; up to three (N,) int64
    ``clears`` are zeroed.  Rows outside the mask are left untouched.  The root record is the reference's root state, every other body is
    carried rigidly by the same transform (include/pulse_hip.h)."""
    from ._lib import TaskResetArgs
    if transform not in TASK_RESET_TRANSFORMS:
        raise ValueError(f"task_ref_state_init: transform must be one of {sorted(TASK_RESET_TRANSFORMS)}, got {transform!r}")
    rb = _dev(rb, "rb")
    n, j = rb.shape[0], motion_lib.num_bodies
    if rb.dim() != 3 or rb.shape[1] != j or rb.shape[2] != 13 or rb.stride(2) != 1 or rb.stride(1) != 13:
        raise ValueError(f"rb: (N, {j}, 13) records with contiguous rows expected, got shape {tuple(rb.shape)} strides {tuple(rb.stride())}")
    nd = 3 * (j - 1)
    f32, i64 = torch.float32, torch.int64
    for t, name, dtype, shape in ((dof_pos, "dof_pos", f32, (n, nd)), (dof_vel, "dof_vel", f32, (n, nd)), (start_times, "start_times", f32, (n,)),
                                  (sampled_ids, "sampled_ids", i64, (n,))) + tuple((c, f"clears[{i}]", i64, (n,)) for i, c in enumerate(clears)):
        _dev(t, name, dtype)
        if tuple(t.shape) != shape or not t.is_contiguous():              # outputs: a temporary copy would swallow the result
            raise ValueError(f"{name}: contiguous {shape} expected, got shape {tuple(t.shape)} strides {tuple(t.stride())}")
    if len(clears) > 3:
        raise ValueError("task_ref_state_init: at most three clears")
    a = TaskResetArgs()
    P = Filler()
    motion_lib.fill_tables(a.tab)
    a.num_envs, a.transform, a.upright_start = n, TASK_RESET_TRANSFORMS[transform], int(bool(upright))
    a.env_mask = P(mask_u8(env_mask), "env_mask", torch.uint8, (n,))
    a.motion_ids, a.times = P(motion_ids, "motion_ids", i64, (n,)), P(times, "times", f32, (n,))
    if transform == "terrain":
        if new_root_xy is None:
            raise TypeError("task_ref_state_init: transform 'terrain' needs new_root_xy")
        a.new_root_xy = P(new_root_xy, "new_root_xy", f32, (n, 2))
        if heightsamples is not None:
            if heightsamples.dtype != torch.int16 or heightsamples.dim() != 2 or not heightsamples.is_contiguous() or not heightsamples.is_cuda:
                raise TypeError("heightsamples: contiguous (rows, cols) int16 CUDA tensor expected")
            if center_points is None:
                raise TypeError("task_ref_state_init: transform 'terrain' over a height field needs center_points")
            a.heightsamples, a.map_rows, a.map_cols = heightsamples.data_ptr(), heightsamples.shape[0], heightsamples.shape[1]
            a.center_points, a.num_center_points = P(center_points, "center_points", f32, (center_points.shape[0], 2)), center_points.shape[0]
        a.horizontal_scale, a.vertical_scale = float(horizontal_scale), float(vertical_scale)
    a.rb, a.rb_env_stride = rb.data_ptr(), rb.stride(0)
    a.dof_pos, a.dof_vel, a.start_times, a.sampled_ids = dof_pos.data_ptr(), dof_vel.data_ptr(), start_times.data_ptr(), sampled_ids.data_ptr()
    for i, c in enumerate(clears):
        setattr(a, f"clear{i}", c.data_ptr())
    _launch("pulse_task_ref_state_init", ctypes.byref(a))


# --------------------------------------------------------------------------- #
# GAE
# --------------------------------------------------------------------------- #
def discount_values(mb_fdones, mb_values, mb_rewards, mb_next_values, gamma, tau, return_returns=False):
    """CommonAgent.discount_values, phc/learning/common_agent.py:493-505.

    Tensors are (T, N, 1) [dones (T, N), uint8 or float] in ANY strides that all agree
    (the reference's time-major layout or this framework's env-major buffers viewed time-major).
    """
    r = _dev(mb_rewards, "mb_rewards")
    t, n = r.shape[0], r.shape[1]
    v, nv = _dev(mb_values, "mb_values"), _dev(mb_next_values, "mb_next_values")
    d = mb_fdones
    if d.dtype != torch.uint8:
        d = (d != 0).to(torch.uint8)
    _dev(d, "mb_fdones", torch.uint8)
    st, sn = r.stride()[0], r.stride()[1]
    for x, name in ((v, "values"), (nv, "next_values")):
        if (x.stride()[0], x.stride()[1]) != (st, sn) or x.shape[:2] != r.shape[:2]:
            raise ValueError(f"discount_values: {name} layout differs from rewards")
    if (d.stride()[0], d.stride()[1]) != (st, sn):
        # bring dones to the rewards' layout (uint8, tiny)
        d2 = torch.empty_strided((t, n), (st, sn), dtype=torch.uint8, device=r.device)
        d2.copy_(d.reshape(t, n))
        d = d2
    advs = torch.empty_strided(r.shape, r.stride(), dtype=torch.float32, device=r.device)
    rets = torch.empty_strided(r.shape, r.stride(), dtype=torch.float32, device=r.device) if return_returns else None
    gt = float(gamma) * float(tau)  # Python evaluates gamma * tau in double first
    _launch("pulse_gae", _ptr(r), _ptr(v), _ptr(nv), _ptr(d), t, n, st, sn, float(gamma), gt, _ptr(advs), _ptr(rets))
    return (advs, rets) if return_returns else advs


# --------------------------------------------------------------------------- #
# trajectory following over a height field (HumanoidTraj / HumanoidPedestrianTerrain)
# --------------------------------------------------------------------------- #
def traj_generate(rb, verts, u_dtheta, u_sharp, sharp_mask, u_heading, u_dspeed, u_speed0, *, episode_dur, dtheta_max=2.0, speed_min=0.0,
                  speed_max=3.0, accel_max=2.0, env_mask=None):
    """TrajGenerator.reset (phc/utils/traj_generator.py:60-123) for the masked envs from uniform draws in the reference's order.
    ``verts`` (N, num_verts, 3) is updated in place; trajectories start at each env's root xy."""
    from ._lib import TrajGenArgs
    rb, verts = _dev(rb, "rb"), _dev(verts, "verts")
    n, nv = verts.shape[0], verts.shape[1]
    if not verts.is_contiguous() or verts.shape[2] != 3:
        raise ValueError("verts: contiguous (N, num_verts, 3) expected")
    seg_dt = episode_dur / (nv - 1)
    a = TrajGenArgs()
    P = Filler()
    f32, u8, seg = torch.float32, torch.uint8, (n, nv - 1)
    a.num_envs, a.num_verts = n, nv
    if env_mask is not None:
        a.env_mask = P(mask_u8(env_mask), "env_mask", u8, (n,))
    a.rb, a.rb_env_stride = rb.data_ptr(), rb.stride(0)
    if any(t is None for t in (u_dtheta, u_sharp, sharp_mask, u_heading, u_dspeed, u_speed0)):
        raise TypeError("traj_generate: every draw is required")
    a.u_dtheta, a.u_sharp, a.u_dspeed = P(u_dtheta, "u_dtheta", f32, seg), P(u_sharp, "u_sharp", f32, seg), P(u_dspeed, "u_dspeed", f32, seg)
    a.sharp_mask = P(mask_u8(sharp_mask), "sharp_mask", u8, seg)
    a.u_heading, a.u_speed0 = P(u_heading, "u_heading", f32, (n,)), P(u_speed0, "u_speed0", f32, (n,))
    a.dtheta_scale, a.dspeed_scale, a.seg_dt = float(dtheta_max * seg_dt), float(accel_max * seg_dt), float(seg_dt)
    a.speed_min, a.speed_max = float(speed_min), float(speed_max)
    a.verts = verts.data_ptr()
    _launch("pulse_traj_generate", ctypes.byref(a))
    return verts


def traj_step(rb, verts, progress, *, what, dt, episode_dur, num_samples=10, sample_timestep=0.5, upright=True, heightsamples=None,
              horizontal_scale=0.1, vertical_scale=0.005, height_points=None, sensor_body=0, center_points=None, use_center_height=True,
              height_meas_scale=5.0, dof_force=None, dof_vel=None, power_coef=0.0005, power_reward=False, fuzzy_target=False, contact_forces=None,
              contact_body_ids=None, termination_heights=None, max_episode_length=300.0, fail_dist=4.0, enable_early_termination=True,
              terrain_reset=True, disable_collision=False, obs=None, obs_offset=0, rew=None, rew_raw=None, reset=None, terminate=None,
              env_ids=None, env_mask=None):
    """One launch of pulse_traj_step (include/pulse_hip.h 2a''): task observation [10 trajectory samples x 2 | height map], location (+ power)
    reward, reset / terminate.  ``height_points`` None = no terrain observation (HumanoidTraj); ``heightsamples`` None with height points =
    terrainType 'plane'.  Returns dict(obs, rew, rew_raw, reset, terminate) of what was asked."""
    from ._lib import TASK_OBS, TASK_RESET, TASK_REWARD, TrajStepArgs
    rb = _dev(rb, "rb")
    n, j = rb.shape[0], rb.shape[1]
    dev = rb.device
    a = TrajStepArgs()
    P = Filler()
    a.what, a.num_envs = what, n
    select_envs(a, P, env_ids, env_mask)
    a.rb, a.rb_env_stride, a.num_bodies, a.upright_start = rb.data_ptr(), rb.stride(0), j, int(bool(upright))
    a.progress, a.dt = P(progress, "progress", torch.int64), float(dt)
    verts = _dev(verts, "verts")
    if verts.shape[0] != n or verts.dim() != 3 or verts.shape[2] != 3 or not verts.is_contiguous():
        raise ValueError("verts: contiguous (N, num_verts, 3) expected")
    nv = verts.shape[1]
    a.verts, a.num_verts, a.traj_dur = verts.data_ptr(), nv, float(nv * (episode_dur / (nv - 1)))
    a.num_samples, a.sample_timestep = int(num_samples), float(sample_timestep)
    nh = 0
    if height_points is not None:
        nh = height_points.shape[0]
        a.height_points, a.num_height_points, a.sensor_body = P(height_points, "height_points"), nh, int(sensor_body)
        if heightsamples is not None:
            if heightsamples.dtype != torch.int16 or heightsamples.dim() != 2 or not heightsamples.is_contiguous() or not heightsamples.is_cuda:
                raise TypeError("heightsamples: contiguous (rows, cols) int16 CUDA tensor expected")
            a.heightsamples, a.map_rows, a.map_cols = heightsamples.data_ptr(), heightsamples.shape[0], heightsamples.shape[1]
        a.horizontal_scale, a.vertical_scale = float(horizontal_scale), float(vertical_scale)
        if center_points is not None:
            a.center_points, a.num_center_points = P(center_points, "center_points"), center_points.shape[0]
        a.use_center_height, a.height_meas_scale = int(bool(use_center_height)), float(height_meas_scale)
    a.dof_force, a.dof_vel = P(dof_force, "dof_force"), P(dof_vel, "dof_vel")
    a.num_dof = dof_force.shape[-1] if dof_force is not None else 0
    a.power_coef, a.power_reward, a.fuzzy_target = float(power_coef), int(bool(power_reward)), int(bool(fuzzy_target))
    if contact_body_ids is not None:
        a.contact_body_ids, a.num_contact_ids = P.ids32(contact_body_ids, "contact_body_ids", dev)
    a.contact_forces, a.termination_heights = P(contact_forces, "contact_forces"), P(termination_heights, "termination_heights")
    a.max_episode_length, a.fail_dist = float(max_episode_length), float(fail_dist)
    a.enable_early_termination, a.terrain_reset, a.disable_collision = int(bool(enable_early_termination)), int(bool(terrain_reset)), int(bool(disable_collision))
    out = {}
    if what & TASK_OBS:
        w = 2 * int(num_samples) + nh
        if obs is None:
            obs = torch.zeros(n, (obs_offset + w + 3) // 4 * 4, dtype=torch.float32, device=dev)
        _dev(obs, "obs")
        a.obs, a.obs_stride, a.obs_offset = obs.data_ptr(), obs.stride(0), int(obs_offset)
        out["obs"] = obs
    step_outputs(a, P, out, n, dev, reward=what & TASK_REWARD, resets=what & TASK_RESET, raw_width=2, rew=rew, rew_raw=rew_raw, reset=reset,
                 terminate=terminate)
    _launch("pulse_traj_step", ctypes.byref(a))
    return out


# --------------------------------------------------------------------------- #
# crowd variant of the terrain task (include/pulse_hip.h section 2a''')
# --------------------------------------------------------------------------- #
def _crowd_rb(rb, group_size, min_group=1):
    rb = _dev(rb, "rb")
    if rb.dim() != 3 or rb.shape[2] != 13 or rb.stride(2) != 1 or rb.stride(1) != 13:
        raise ValueError(f"rb: (N, J, 13) rigid-body records with packed bodies expected, got shape {tuple(rb.shape)} strides {tuple(rb.stride())}")
    n, g = rb.shape[0], int(group_size)
    if g < min_group:
        raise ValueError(f"group_size = {g} < {min_group}" + (": the reference takes the 6 smallest group distances (torch.topk, "
                         "humanoid_pedestrian_terrain.py:1724)" if min_group > 1 else ""))
    if n % g != 0:
        raise ValueError(f"num_envs = {n} is not a multiple of group_size = {g} (the reference's group ids, humanoid.py:259-261, have no meaning there)")
    return rb, n, g


def crowd_group_obs(rb, group_size, *, upright=True, obs=None, obs_offset=0, env_ids=None, env_mask=None):
    """compute_group_observation (humanoid_pedestrian_terrain.py:1700-1753): one launch of pulse_crowd_group_obs.  ``rb`` (N, J >= 24, 13);
    envs are grouped contiguously by ``group_size`` (>= 6).  Writes 165 floats per selected env at ``obs[:, obs_offset:]`` (allocated when
    None) and returns ``obs``."""
    from ._lib import CROWD_GROUP_OBS, CrowdGroupObsArgs
    rb, n, g = _crowd_rb(rb, group_size, 6)
    if rb.shape[1] < 24:
        raise ValueError(f"rb: the neighbour observation reads bodies up to index 23, got {rb.shape[1]} bodies")
    a, P = CrowdGroupObsArgs(), Filler()
    a.num_envs, a.group_size = n, g
    select_envs(a, P, env_ids, env_mask)
    a.rb, a.rb_env_stride, a.num_bodies, a.upright_start = rb.data_ptr(), rb.stride(0), rb.shape[1], int(bool(upright))
    if obs is None:
        obs = torch.zeros(n, (obs_offset + CROWD_GROUP_OBS + 3) // 4 * 4, dtype=torch.float32, device=rb.device)
    a.obs, a.obs_stride = rows2d(obs, "obs", n, obs_offset + CROWD_GROUP_OBS)
    a.obs_offset = int(obs_offset)
    _launch("pulse_crowd_group_obs", ctypes.byref(a))
    return obs


def _crowd_map(heightsamples):
    if not isinstance(heightsamples, torch.Tensor) or heightsamples.dtype != torch.int16 or heightsamples.dim() != 2 or not heightsamples.is_contiguous() \
            or not heightsamples.is_cuda:
        raise TypeError("heightsamples: contiguous (rows, cols) int16 CUDA tensor expected")
    return heightsamples.shape[0], heightsamples.shape[1]


def crowd_stamp(rb, group_size, owner, cells, *, horizontal_scale=0.1, clear=True):
    """People into the height map (get_heights :749-761, sample_height_points :1207-1221): every person's 10 x 20 root-point footprint marks
    ``owner`` (num_groups, rows, cols) int32 with its env index + 1 (the highest index wins a shared cell) and lists its cells in ``cells``
    (N, 200) int32.  ``clear``: first empty the cells ``cells`` lists from the previous call (fill it with -1 before the first).  Returns
    ``owner``."""
    from ._lib import CROWD_ROOT_POINTS, CrowdStampArgs
    rb, n, g = _crowd_rb(rb, group_size)
    _dev(owner, "owner", torch.int32), _dev(cells, "cells", torch.int32)
    if owner.dim() != 3 or owner.shape[0] != n // g or not owner.is_contiguous():
        raise ValueError(f"owner: contiguous ({n // g}, rows, cols) int32 expected, got {tuple(owner.shape)}")
    if tuple(cells.shape) != (n, CROWD_ROOT_POINTS) or not cells.is_contiguous():
        raise ValueError(f"cells: contiguous ({n}, {CROWD_ROOT_POINTS}) int32 expected, got {tuple(cells.shape)}")
    a = CrowdStampArgs()
    a.num_envs, a.group_size, a.rb, a.rb_env_stride = n, g, rb.data_ptr(), rb.stride(0)
    a.map_rows, a.map_cols, a.horizontal_scale = owner.shape[1], owner.shape[2], float(horizontal_scale)
    a.owner, a.cells, a.clear = owner.data_ptr(), cells.data_ptr(), int(bool(clear))
    _launch("pulse_crowd_stamp", ctypes.byref(a))
    return owner


def crowd_heights(rb, heightsamples, height_points, *, group_size=0, owner=None, velocity_map=False, upright=True, sensor_body=0,
                  center_points=None, use_center_height=False, horizontal_scale=0.1, vertical_scale=0.005, height_meas_scale=5.0, obs=None,
                  obs_offset=0, env_ids=None, env_mask=None):
    """The height block of the crowd / velocity modes (get_heights :718-772, sample_height_points :1200-1276, tail of _compute_task_obs
    :414-427): one launch of pulse_crowd_heights.  ``owner`` (from crowd_stamp) raises stamped cells by short(1.7 / vertical_scale) and, with
    ``velocity_map``, supplies each sample's velocity; ``velocity_map`` makes the block (N, 3 * P) interleaved [h, vx, vy].  Writes at
    ``obs[:, obs_offset:]`` (allocated when None) and returns ``obs``."""
    from ._lib import CrowdHeightsArgs
    rb, n, g = _crowd_rb(rb, group_size if owner is not None else 1)
    rows, cols = _crowd_map(heightsamples)
    a, P = CrowdHeightsArgs(), Filler()
    a.num_envs, a.group_size = n, g
    select_envs(a, P, env_ids, env_mask)
    a.rb, a.rb_env_stride, a.num_bodies, a.upright_start = rb.data_ptr(), rb.stride(0), rb.shape[1], int(bool(upright))
    a.heightsamples, a.map_rows, a.map_cols = heightsamples.data_ptr(), rows, cols
    a.horizontal_scale, a.vertical_scale = float(horizontal_scale), float(vertical_scale)
    if owner is not None:
        _dev(owner, "owner", torch.int32)
        if tuple(owner.shape) != (n // g, rows, cols) or not owner.is_contiguous():
            raise ValueError(f"owner: contiguous ({n // g}, {rows}, {cols}) int32 expected, got {tuple(owner.shape)}")
        a.owner = owner.data_ptr()
    a.stamp_raise = int(ctypes.c_float(1.7 / float(vertical_scale)).value)                # torch.tensor(1.7 / vertical_scale).short(), :1226
    nh = height_points.shape[0]
    a.height_points, a.num_height_points, a.sensor_body = P(height_points, "height_points", shape=(nh, 2)), nh, int(sensor_body)
    if center_points is not None:
        a.center_points, a.num_center_points = P(center_points, "center_points"), center_points.shape[0]
    a.use_center_height, a.height_meas_scale, a.velocity_map = int(bool(use_center_height)), float(height_meas_scale), int(bool(velocity_map))
    w = (3 if velocity_map else 1) * nh
    if obs is None:
        obs = torch.zeros(n, (obs_offset + w + 3) // 4 * 4, dtype=torch.float32, device=rb.device)
    a.obs, a.obs_stride = rows2d(obs, "obs", n, obs_offset + w)
    a.obs_offset = int(obs_offset)
    _launch("pulse_crowd_heights", ctypes.byref(a))
    return obs


# --------------------------------------------------------------------------- #
# the walkable map of the terrain task (include/pulse_hip.h section 2a'''')
# --------------------------------------------------------------------------- #
def _terrain_grid(t, name, dtype, shape=None):
    _dev(t, name, dtype)
    if t.dim() != 2 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = "(rows, cols)" if shape is None else str(tuple(shape))
        raise ValueError(f"{name}: contiguous {want} {dtype} expected, got shape {tuple(t.shape)} strides {tuple(t.stride())}")
    return t


def terrain_walkable(heights=None, *, tile_flags=None, border=0, length_px=0, width_px=0, obstacle_mask=None, iterations=3, out=None):
    """The obstacle field of Terrain (humanoid_pedestrian_terrain.py:1362-1364, 1380, 1443-1445, 1471) in one launch of pulse_terrain_walkable:
    (rows, cols) uint8, 1 where a cell of a flagged tile with a non-zero height -- or a set cell of ``obstacle_mask`` -- lies within L1
    distance ``iterations`` (ndimage.binary_dilation's default cross, zero border).  ``heights`` (rows, cols) int16 with ``tile_flags``
    (tile_rows, tile_cols) uint8 / bool; tile (i, j) starts at row border + i * length_px, column border + j * width_px."""
    from ._lib import TerrainWalkableArgs
    if tile_flags is None and obstacle_mask is None:
        raise TypeError("terrain_walkable: tile_flags (with heights) or obstacle_mask is required")
    a, P = TerrainWalkableArgs(), Filler()
    shape = None
    if tile_flags is not None:
        if heights is None:
            raise TypeError("terrain_walkable: tile_flags need heights")
        shape = tuple(_terrain_grid(heights, "heights", torch.int16).shape)
        flags = _terrain_grid(mask_u8(tile_flags), "tile_flags", torch.uint8)
        a.heights, a.tile_flags, a.tile_rows, a.tile_cols = heights.data_ptr(), P(flags, "tile_flags", torch.uint8), flags.shape[0], flags.shape[1]
        a.border, a.length_px, a.width_px = int(border), int(length_px), int(width_px)
    if obstacle_mask is not None:
        mask = _terrain_grid(mask_u8(obstacle_mask), "obstacle_mask", torch.uint8, shape)
        shape = tuple(mask.shape)
        a.obstacle_mask = P(mask, "obstacle_mask", torch.uint8)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=(heights if heights is not None else obstacle_mask).device)
    _terrain_grid(out, "out", torch.uint8, shape)
    a.rows, a.cols, a.iterations, a.walkable = shape[0], shape[1], int(iterations), out.data_ptr()
    _launch("pulse_terrain_walkable", ctypes.byref(a))
    return out


def terrain_valid_cells(walkable, *, border_scaled, horizontal_scale=0.1, coord_x=None, coord_y=None):
    """The table of valid start cells (Terrain.__init__ :1160-1172) from a (rows, cols) uint8 walkable field: the cells with value 0 that lie
    more than ``border_scaled`` (the host's float32 border * horizontal_scale) inside the candidates' own extent, scaled to metres, in
    torch.where's order.  ``coord_x`` / ``coord_y``: equally long float32 buffers to fill -- entries past the count are not touched, cells past
    the buffers' end are dropped; None: count only (size the table from it and call again).  Returns (coord_x, coord_y, count) with ``count``
    a device int64 of one element: nothing is read back here."""
    from ._lib import TerrainValidArgs
    w = _terrain_grid(mask_u8(walkable), "walkable", torch.uint8)
    rows, cols = w.shape
    dev = w.device
    if (coord_x is None) != (coord_y is None):
        raise TypeError("terrain_valid_cells: coord_x and coord_y come together")
    if coord_x is not None:
        _dev(coord_x, "coord_x"), _dev(coord_y, "coord_y")
        if coord_x.dim() != 1 or coord_x.shape != coord_y.shape or not (coord_x.is_contiguous() and coord_y.is_contiguous()):
            raise ValueError(f"coord_x / coord_y: equally long contiguous 1-D buffers expected, got {tuple(coord_x.shape)} and {tuple(coord_y.shape)}")
    extents = torch.empty(2 * rows + 4, dtype=torch.int32, device=dev)
    offsets = torch.empty(rows + 1, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    a = TerrainValidArgs()
    a.rows, a.cols, a.walkable = rows, cols, w.data_ptr()
    a.horizontal_scale, a.border_scaled = float(horizontal_scale), float(border_scaled)
    a.row_extents, a.row_offsets = extents.data_ptr(), offsets.data_ptr()
    a.count = count.data_ptr()
    if coord_x is not None and coord_x.numel() > 0:
        a.coord_x, a.coord_y, a.capacity = coord_x.data_ptr(), coord_y.data_ptr(), coord_x.numel()
    _launch("pulse_terrain_valid_cells", ctypes.byref(a))
    return coord_x, coord_y, count


def terrain_sample(out, *, coord_x=None, coord_y=None, idx=None, env_mask=None, group_num_people=0, extent_x=0.0, extent_y=0.0, u_center=None,
                   u_dx=None, u_dy=None):
    """Terrain.sample_valid_locations (:1175-1189) from injected draws, one launch of pulse_terrain_sample: the rows of ``out`` (N, 2) that
    ``env_mask`` selects (all when None) receive (coord_x[idx[e]], coord_y[idx[e]]) -- ``idx`` (N,) int64 in [0, len(coord_x)) -- or, with
    ``group_num_people`` P > 0, centre of group e // P plus member e % P's offset from the uniforms ``u_center`` (2, N / P), ``u_dx`` and
    ``u_dy`` (N / P, P).  The other rows are not touched."""
    from ._lib import TerrainSampleArgs
    _dev(out, "out")
    if out.dim() != 2 or out.shape[1] != 2 or not out.is_contiguous():
        raise ValueError(f"out: contiguous (N, 2) expected, got shape {tuple(out.shape)} strides {tuple(out.stride())}")
    n, p = out.shape[0], int(group_num_people)
    a, P = TerrainSampleArgs(), Filler()
    a.num_envs, a.out, a.group_num_people = n, out.data_ptr(), p
    if env_mask is not None:
        a.env_mask = P(mask_u8(env_mask), "env_mask", torch.uint8, (n,))
    if p > 0:
        if n % p != 0:
            raise ValueError(f"terrain_sample: {n} envs are not a multiple of group_num_people {p}")
        if u_center is None or u_dx is None or u_dy is None:
            raise TypeError("terrain_sample: group mode needs u_center, u_dx and u_dy")
        g = n // p
        a.u_center, a.u_dx, a.u_dy = P(u_center, "u_center", shape=(2, g)), P(u_dx, "u_dx", shape=(g, p)), P(u_dy, "u_dy", shape=(g, p))
        a.extent_x, a.extent_y = float(extent_x), float(extent_y)
    else:
        if coord_x is None or coord_y is None or idx is None:
            raise TypeError("terrain_sample: coord_x, coord_y and idx are required")
        m = coord_x.shape[0]
        a.coord_x, a.coord_y, a.num_samples = P(coord_x, "coord_x", shape=(m,)), P(coord_y, "coord_y", shape=(m,)), m
        a.idx = P(idx, "idx", torch.int64, (n,))
    _launch("pulse_terrain_sample", ctypes.byref(a))
    return out


# --------------------------------------------------------------------------- #
# MCP composer stage (include/pulse_hip.h section 4e)
# --------------------------------------------------------------------------- #
def mcp_compose(weights, x, out=None, *, num_actions=None, discrete=False):
    """HumanoidImMCP.step's mixture (phc/env/tasks/humanoid_im_mcp.py:56-67): ``weights`` (N, P), ``x`` (N, P, a_pitch) -- the primitives'
    outputs side by side, rows may be pitched views -- -> actions (N, num_actions) = sum_k weights[:, k, None] * x[:, k, :num_actions].
    ``discrete``: the weight row becomes one_hot(argmax) first (:56-58)."""
    _dev(weights, "weights"), _dev(x, "x")
    if x.dim() != 3 or weights.dim() != 2 or x.shape[0] != weights.shape[0] or x.shape[1] != weights.shape[1]:
        raise ValueError(f"mcp_compose: weights (N, P) and x (N, P, a_pitch) expected, got {tuple(weights.shape)} and {tuple(x.shape)}")
    n, p = weights.shape
    wp, ws = rows2d(weights, "weights", n, p)
    if x.numel() > 0 and (x.stride(2) != 1 or x.stride(1) < x.shape[2] or (n > 1 and x.stride(0) < p * x.stride(1))):
        raise ValueError(f"x: expected (N, P, a_pitch) rows with unit inner stride, got strides {tuple(x.stride())}")
    a = int(num_actions) if num_actions is not None else x.shape[2]
    if not 1 <= a <= x.shape[2]:
        raise ValueError(f"mcp_compose: num_actions = {a} outside 1 .. {x.shape[2]}")
    if out is None:
        out = torch.empty(n, a, dtype=torch.float32, device=x.device)
    op, os_ = rows2d(out, "out", n, a)
    _launch("pulse_mcp_compose", wp, ws, _ptr(x), x.stride(0) if n else p * x.stride(1), x.stride(1), n, p, a, int(bool(discrete)), op, os_)
    return out[:, :a]


# --------------------------------------------------------------------------- #
# Actuation stage (include/pulse_hip.h section 4f)
# --------------------------------------------------------------------------- #
def pd_targets(action, scale, *, clip=float("inf"), offset=None, freeze=None, ref_dof_pos=None, sim_dof_pos=None, clamped=None, target=None):
    """The env step's actuation stage in one launch (the agent's action clamp, phc/learning/im_amp.py:68-73; Humanoid.pre_physics_step,
    phc/env/tasks/humanoid.py:1222-1247; _action_to_pd_targets, humanoid.py:1392-1394 and humanoid_im.py:1096-1101): ``action`` (N, D), rows may
    be a pitched view -> (clamped, target), both (N, D) (allocated when None; pitched views are written in their first D columns only).
    clamped = clamp(action, -clip, clip); target = offset + scale * clamped, or with ``ref_dof_pos`` / ``sim_dof_pos`` (res_action) ref + scale *
    clamped held inside sim_dof_pos -+ pi / 2; columns whose ``freeze`` byte is set get target 0.  ``offset`` / ``scale`` (D,) float32, ``freeze``
    (D,) uint8 / bool."""
    _dev(action, "action")
    if action.dim() != 2:
        raise ValueError(f"pd_targets: action (N, D) expected, got {tuple(action.shape)}")
    n, d = action.shape
    clip = float(clip)
    if not clip >= 0.0:
        raise ValueError(f"pd_targets: clip = {clip!r}: a bound >= 0 (inf for none)")
    if (ref_dof_pos is None) != (sim_dof_pos is None):
        raise ValueError("pd_targets: the residual form takes ref_dof_pos and sim_dof_pos together")
    P = Filler()
    ap, as_ = rows2d(action, "action", n, d)
    sp = P(scale, "scale", shape=(d,))
    op = P(offset, "offset", shape=(d,))
    fp = P(None if freeze is None else mask_u8(freeze), "freeze", torch.uint8, shape=(d,))
    rp, rs, mp, ms = None, 0, None, 0
    if ref_dof_pos is not None:
        rp, rs = rows2d(ref_dof_pos, "ref_dof_pos", n, d)
        mp, ms = rows2d(sim_dof_pos, "sim_dof_pos", n, d)
    if clamped is None:
        clamped = torch.empty(n, d, dtype=torch.float32, device=action.device)
    if target is None:
        target = torch.empty(n, d, dtype=torch.float32, device=action.device)
    cp, cs = rows2d(clamped, "clamped", n, d)
    tp, ts = rows2d(target, "target", n, d)
    _launch("pulse_pd_targets", ap, as_, n, d, clip, op, sp, fp, rp, rs, mp, ms, cp, cs, tp, ts)
    return clamped[:, :d], target[:, :d]
