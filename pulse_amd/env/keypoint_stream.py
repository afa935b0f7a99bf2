"""A reference that arrives one frame at a time: 3-D keypoints from a video pose estimator, a text-to-motion model or a headset, filtered on the
device into the ``ref_next`` of the imitation step.

What HumanoidImMCPDemo does on the host every control step (phc/env/tasks/humanoid_im_mcp_demo.py:252-290: numpy reorder and rescale, three
deque(maxlen=30), scipy's gaussian_filter1d over the whole history three times to keep one sample, finite-difference velocity, upload) is ONE
launch of ``pulse_keypoint_push`` (csrc/keypoint_stream.hip, include/pulse_hip.h section 2b'.3) per pushed frame; the rings, the per-env push
counts and the previous positions live on the device.  The caller owns the transport: nothing here opens a socket.

``KeypointStream`` plays RecordedMotion's part for HumanoidIm (a reference source without ``query``): ``next()`` / ``next_after_reset()`` hand
out views of its two output buffers -- always the same storage, so the env's cached ``pulse_im_step`` launch stays valid across pushes.
A coincident keypoint set (all joints at one point) has limb scale 0: its positions are 0 / 0 = NaN, as the reference's numpy gives, and stay
NaN while the frame is in the env's history (``clear`` drops it).  A validity mask for dropped detections is not built.
"""
import torch

from .. import kernels
from .. import synthetic as syn

LARGE_MOTION_LENGTH = 1.0e9          # seconds: a stream never runs out


class KeypointStream:
    def __init__(self, num_envs, device, history=30, sigmas=(10, 5, 2), dt=1.0 / 30.0, joint_map=None, frame="y_up", parents=None):
        """``history``: the reference's deque length (1 .. 64); ``sigmas``: root component 2, root components 0 / 1, body coordinates
        (humanoid_im_mcp_demo.py:278-284); ``dt``: the stream's frame period s_dt (:274); ``joint_map``: body -> input joint, default
        smpl_2_mujoco (:32); ``frame``: "y_up" applies the reference's to_isaac_mat (:56), "sim" takes keypoints already in the simulator's
        frame.  The options are validated before any device buffer exists."""
        self.history = check_history(history)
        if len(sigmas) != 3:
            raise ValueError(f"KeypointStream: sigmas {sigmas!r}: three are expected (root component 2, root components 0 / 1, bodies)")
        taps = kernels.keypoint_taps(tuple(float(s) for s in sigmas), self.history)
        self._frame = kernels.keypoint_frame(frame)
        if not float(dt) > 0:
            raise ValueError(f"KeypointStream: dt {dt!r} must be positive")
        self.joint_map = list(syn.smpl_joint_map() if joint_map is None else joint_map)
        self.parents = list(syn.SMPL_PARENTS if parents is None else parents)
        if len(self.joint_map) != len(self.parents) or sorted(self.joint_map) != list(range(len(self.parents))):
            raise ValueError(f"KeypointStream: joint_map must be a permutation of 0 .. {len(self.parents) - 1}")
        self.num_envs, self.num_bodies, self.dt, self.device = int(num_envs), len(self.parents), float(dt), torch.device(device)
        n, j, h, dev = self.num_envs, self.num_bodies, self.history, self.device
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=dev)
        self.taps = torch.from_numpy(taps).to(torch.float32).to(dev)                    # built in float64, cast once, uploaded once
        self.root_ring, self.body_ring = z(n, h, 3), z(n, h, j, 3)
        self.count = torch.zeros(n, dtype=torch.int32, device=dev)
        self.prev_pos, self.pos, self.vel, self.raw = z(n, j, 3), z(n, j, 3), z(n, j, 3), z(n, j, 3)
        self._out = {"pos": self.pos, "vel": self.vel}
        self._motion_lengths = torch.full((n,), LARGE_MOTION_LENGTH, dtype=torch.float32, device=dev)
        self.device = self.count.device                                                 # with its index, as tensors report it
        self.pushes = 0

    # ------------------------------------------------------------------ feeding
    def push(self, j3d, env_mask=None):
        """One frame of keypoints (N, J, 3) float32 on the stream's device, input joint order, inner stride 1 -> the filtered reference in
        ``pos`` / ``vel``; one launch.  ``env_mask`` (N,) bool: envs at False keep their state and outputs."""
        check_keypoints(j3d, self.num_envs, self.num_bodies, self.device)
        if env_mask is not None and (not isinstance(env_mask, torch.Tensor) or tuple(env_mask.shape) != (self.num_envs,) or
                                     env_mask.dtype not in (torch.bool, torch.uint8) or env_mask.device != self.device):
            raise ValueError(f"KeypointStream.push: env_mask must be a ({self.num_envs},) bool tensor on {self.device}")
        kernels.keypoint_push(j3d, taps=self.taps, root_ring=self.root_ring, body_ring=self.body_ring, count=self.count, prev_pos=self.prev_pos,
                              pos=self.pos, vel=self.vel, raw=self.raw, joint_map=self.joint_map, parents=self.parents, env_mask=env_mask,
                              frame=self._frame, dt=self.dt)
        self.pushes += 1
        return self._out

    def direct(self, pos, vel):
        """HumanoidImDemo's form (humanoid_im_demo.py:147-152): positions and velocities taken as given -- body order, simulator frame, no
        filter.  (N, J, 3) or (1, J, 3) (the reference's single j3d row serves every env), copied into the output buffers."""
        for name, t in (("pos", pos), ("vel", vel)):
            if not isinstance(t, torch.Tensor) or t.dim() != 3 or tuple(t.shape[1:]) != (self.num_bodies, 3) or t.shape[0] not in (1, self.num_envs):
                raise ValueError(f"KeypointStream.direct: {name} must be a ({self.num_envs} | 1, {self.num_bodies}, 3) tensor")
        self.pos.copy_(pos.to(self.device, torch.float32).expand_as(self.pos))
        self.vel.copy_(vel.to(self.device, torch.float32).expand_as(self.vel))
        return self._out

    def clear(self, env_mask=None):
        """Forget the history of the masked envs (default: all): count and prev_pos to zero, so their next push is a first push."""
        if env_mask is None:
            self.count.zero_()
            self.prev_pos.zero_()
        else:
            self.count.masked_fill_(env_mask, 0)
            self.prev_pos.masked_fill_(env_mask[:, None, None], 0.0)

    # ------------------------------------------------------------------ RecordedMotion's surface
    def next(self):
        return self._out

    def next_after_reset(self):
        return self._out

    def now(self):
        raise NotImplementedError("KeypointStream.now: a streamed reference has no frame for the current state -- the demo tasks compute no "
                                  "reward and no reset (humanoid_im_mcp_demo.py:319-321)")

    def sample_demo_states(self, count):
        raise NotImplementedError("KeypointStream.sample_demo_states: a streamed reference has no motion to draw AMP demonstrations from "
                                  "(enable_amp_obs is not built for the demo tasks)")


def check_history(history):
    h = int(history)
    if h != history or not 1 <= h <= kernels.KEYPOINT_MAX_HISTORY:
        raise ValueError(f"KeypointStream: history {history!r} not in [1, {kernels.KEYPOINT_MAX_HISTORY}]")
    return h


def check_keypoints(j3d, num_envs, num_bodies, device):
    """A frame of the wrong shape, dtype, device or layout is a ValueError before anything is launched.  Needs no device."""
    if not isinstance(j3d, torch.Tensor):
        raise ValueError(f"KeypointStream.push: j3d must be a torch.Tensor, got {type(j3d).__name__}")
    if tuple(j3d.shape) != (num_envs, num_bodies, 3):
        raise ValueError(f"KeypointStream.push: j3d must have shape ({num_envs}, {num_bodies}, 3), got {tuple(j3d.shape)}")
    if j3d.dtype != torch.float32:
        raise ValueError(f"KeypointStream.push: j3d must be float32, got {j3d.dtype}")
    if j3d.device != torch.device(device):
        raise ValueError(f"KeypointStream.push: j3d must live on {device}, got {j3d.device}")
    if j3d.stride(-1) != 1 or j3d.stride(1) < 3 or j3d.stride(0) < 0:
        raise ValueError(f"KeypointStream.push: j3d needs unit inner stride and at least 3 floats between joints, got strides {tuple(j3d.stride())}")
