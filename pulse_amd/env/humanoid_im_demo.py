"""HumanoidImMCPDemo / HumanoidImDemo on MI355X: a trained tracker driven by keypoints that arrive one frame at a time.

Mirrors phc/env/tasks/humanoid_im_mcp_demo.py (HumanoidImMCPDemo: __init__ :37-66, _compute_observations :128-154, _compute_task_obs_demo
:156-317, _compute_reset :319-321) and phc/env/tasks/humanoid_im_demo.py (HumanoidImDemo: :24-27, 98-169):

  reference                                                     here
  requests.get(...)/ws message per control step                 the caller's: ``push_keypoints(j3d)`` (or ``stream.direct(pos, vel)``); no socket is opened
  numpy reorder, limb scale, three deques, three scipy filters   one launch of pulse_keypoint_push (env/keypoint_stream.py)
  tracked subset, far masking, compute_imitation_observations_v7 the ordinary pulse_im_step with PULSE_IM_SELF_OBS | PULSE_IM_TASK_OBS, the stream's buffers
                                                                as ``ref_next`` and zero_out_far (close_distance 0.5 / 0.25) as the kernel already has it
  _compute_reset: reset_buf[:] = 0, _terminate_buf[:] = 0        no reward / reset stage is launched: rew_buf, reset_buf, _terminate_buf stay zero

Both classes here NEVER reset on their own.  The reference's MCP demo clears its reset flags every step; its plain demo keeps HumanoidIm's reset
against a motion library, which a stream does not have, so that reset is not built.  ``reset()`` / ``reset_masked()`` still re-initialise the
simulator state of the envs the caller names and recompute their observation against the stream's current output; they leave the stream's
history alone (``stream.clear`` is the caller's).
obs_v must be 7 (6 raises in the reference itself, humanoid_im_mcp_demo.py:177-178); fut_tracks and enable_amp_obs raise by name: the demo has no
future frames and no AMP window.  zero_out_far_train is inert (the reference's demo never reaches the code that reads it): the base class gets a
copy of the env dict with it False.
"""
from .._lib import PULSE_IM_SELF_OBS, PULSE_IM_TASK_OBS
from .humanoid_im import HumanoidIm, _env_dict
from .humanoid_im_mcp import HumanoidImMCP
from .keypoint_stream import KeypointStream, check_history

NO_FAR_DISTANCE = float("inf")       # the plain demo has no far-direction clamp (humanoid_im_demo.py:154-160): no distance exceeds this


def check_demo_options(cfg, task="HumanoidImMCPDemo", history=30):
    """The demo's switches of an env dict; raises by name for what the reference does not run or this package does not build.  Needs no device."""
    env = _env_dict(cfg)
    obs_v = int(env.get("obs_v", 6))
    if obs_v == 6:
        raise NotImplementedError(f"{task}: obs_v 6 raises NotImplementedError in the reference itself (humanoid_im_mcp_demo.py:177-178: "
                                  "'use obs_v == 7 instead'); obs_v must be 7")
    if obs_v != 7:
        raise NotImplementedError(f"{task}: obs_v {obs_v}: the streamed reference carries positions and velocities only, obs_v must be 7 "
                                  "(humanoid_im_mcp_demo.py:252-310)")
    if env.get("fut_tracks", False):
        raise NotImplementedError(f"{task}: fut_tracks: a streamed reference has no future frames (time_steps = 1, humanoid_im_mcp_demo.py:292)")
    if env.get("enable_amp_obs", False):
        raise NotImplementedError(f"{task}: enable_amp_obs: the demo has no motion library to initialise an AMP window or draw demonstrations from")
    check_history(history)


def _demo_cfg(cfg):
    """A copy of ``cfg`` whose env dict carries zero_out_far_train = False (module docstring)."""
    cfg = dict(cfg)
    if isinstance(cfg.get("env", None), dict):
        env = dict(cfg["env"])
        if isinstance(env.get("env", None), dict):
            env["env"] = dict(env["env"], zero_out_far_train=False)
        else:
            env["zero_out_far_train"] = False
        cfg["env"] = env
    else:
        cfg["zero_out_far_train"] = False
    return cfg


class _KeypointDemo:
    """What the two demo tasks share: the stream as the reference source, the observation-only step."""

    def _finish_demo(self, close_distance, far_distance=None):
        self.stream = self._motion_lib
        self.close_distance = float(close_distance)                 # set after the base constructor, as the reference does (:65)
        if far_distance is not None:
            self.far_distance = float(far_distance)
        self.reset_buf.zero_()                                      # _compute_reset (:319-321): the flags are never set
        self._terminate_buf.zero_()

    def push_keypoints(self, j3d, env_mask=None):
        """One frame of keypoints (N, 24, 3) for the next observation: forwards to the stream (one launch)."""
        return self.stream.push(j3d, env_mask=env_mask)

    def _compute_reward(self, actions=None):
        return                                                      # the demo has no reward

    def _compute_reset(self):
        self.reset_buf.zero_()
        self._terminate_buf.zero_()

    def post_physics_step(self):
        if self.self_obs_v == 2:
            self._update_tensor_history()
        self.progress_buf += 1
        sink, self._obs_sink = self._obs_sink, None
        self._im_step(PULSE_IM_SELF_OBS | PULSE_IM_TASK_OBS, obs_copy=sink)       # against stream.next(): the same storage every step
        self.obs_sink_written = sink is not None
        self._obs_post()
        self.extras["terminate"] = self._terminate_buf
        self.extras["reward_raw"] = self.reward_raw


def _stream_for(sim, device, stream, history):
    if stream is None:
        return KeypointStream(sim.num_envs, device, history=history)
    if stream.num_envs != sim.num_envs:
        raise ValueError(f"the stream serves {stream.num_envs} envs but the injected simulator has {sim.num_envs}")
    return stream


class HumanoidImMCPDemo(_KeypointDemo, HumanoidImMCP):
    def __init__(self, cfg, sim, stream=None, device="cuda:0", pnn_checkpoint=None, history=30):
        """``stream``: a KeypointStream of the simulator's env count; without one the task builds its own (``history`` frames).
        ``pnn_checkpoint`` as HumanoidImMCP takes it."""
        check_demo_options(cfg, type(self).__name__, history)
        HumanoidImMCP.__init__(self, _demo_cfg(cfg), sim, _stream_for(sim, device, stream, history), device=device, pnn_checkpoint=pnn_checkpoint)
        self._finish_demo(0.5)                                      # humanoid_im_mcp_demo.py:65; far_distance stays the env dict's (:304)


class HumanoidImDemo(_KeypointDemo, HumanoidIm):
    def __init__(self, cfg, sim, stream=None, device="cuda:0", pnn_checkpoint=None, history=30):
        """HumanoidImDemo (humanoid_im_demo.py): positions and velocities usually come as given (``stream.direct``), close_distance is the
        literal 0.25 (:155) and there is no far-direction clamp.  ``pnn_checkpoint`` is accepted for the common signature and must be None."""
        check_demo_options(cfg, type(self).__name__, history)
        if pnn_checkpoint is not None:
            raise ValueError("HumanoidImDemo composes no primitives: pnn_checkpoint belongs to HumanoidImMCPDemo")
        HumanoidIm.__init__(self, _demo_cfg(cfg), sim, _stream_for(sim, device, stream, history), device=device)
        self._finish_demo(0.25, NO_FAR_DISTANCE)
