"""numpy restatement of pulse_keypoint_push (include/pulse_hip.h section 2b'.3): lines 252-290 and 310 of the reference's
HumanoidImMCPDemo._compute_task_obs_demo with a ``dtype`` argument and PER-ENV counts.

``dtype=np.float64`` is the yardstick the kernel is held to; ``dtype=np.float32`` is "float32 staging": every array, every tap and every
accumulation in float32, in the kernel's operation order -- the distance between the two runs is the error of an fp32 evaluation of the
reference's own statements (the rule of tests/test_motion_ingest_gpu.py).  Used by tools/gen_golden_keypoint_stream.py and the tests; needs no
device and no scipy."""
import numpy as np

from pulse_amd import kernels
from pulse_amd import synthetic as syn

LIMBS = 5


class StreamModel:
    def __init__(self, num_envs, history=30, sigmas=(10.0, 5.0, 2.0), dt=1.0 / 30.0, joint_map=None, parents=None, frame="y_up",
                 mean_limb_lengths=kernels.KEYPOINT_MEAN_LIMB_LENGTHS, dtype=np.float64, taps=None):
        self.n, self.h, self.dtype = int(num_envs), int(history), np.dtype(dtype)
        self.joint_map = list(syn.smpl_joint_map() if joint_map is None else joint_map)
        self.parents = list(syn.SMPL_PARENTS if parents is None else parents)
        self.j = len(self.joint_map)
        # the table as the device sees it: built in float64, cast to float32 once (the fp64 run keeps the float64 table)
        t = kernels.keypoint_taps(sigmas, self.h) if taps is None else np.asarray(taps)
        self.taps = t.astype(np.float32).astype(self.dtype) if self.dtype == np.float32 else t.astype(np.float64)
        # the reference keeps mean_limb_lengths, the frame matrix and dt as float32 values
        self.mean = np.asarray(mean_limb_lengths, dtype=np.float32).astype(self.dtype)
        m = kernels.keypoint_frame(frame) if isinstance(frame, str) else np.asarray(frame)
        self.frame = m.astype(np.float32).astype(self.dtype)
        self.dt = np.float32(dt).astype(self.dtype)
        self.root_ring = np.zeros((self.n, self.h, 3), dtype=self.dtype)
        self.body_ring = np.zeros((self.n, self.h, self.j, 3), dtype=self.dtype)
        self.count = np.zeros(self.n, dtype=np.int64)
        self.prev_pos = np.zeros((self.n, self.j, 3), dtype=self.dtype)
        self.pos = np.zeros((self.n, self.j, 3), dtype=self.dtype)
        self.vel = np.zeros((self.n, self.j, 3), dtype=self.dtype)
        self.raw = np.zeros((self.n, self.j, 3), dtype=self.dtype)

    def clear(self, env_mask=None):
        sel = np.ones(self.n, dtype=bool) if env_mask is None else np.asarray(env_mask, dtype=bool)
        self.count[sel] = 0
        self.prev_pos[sel] = 0

    def _filter(self, ring, e, w, length, table):
        """sum_{i < L} taps[table, L - 1, i] * history[i], oldest first; ``ring`` (H, ...) of env e, ``table`` per trailing coordinate."""
        acc = np.zeros(ring.shape[1:], dtype=self.dtype)
        for i in range(length):
            s = (w - (length - 1 - i)) % self.h
            acc = acc + self.taps[table, length - 1, i] * ring[s]
        return acc

    def push(self, j3d, env_mask=None):
        """One frame (N, J, 3), any float dtype (cast to the run's).  -> views of pos, vel."""
        d = self.dtype
        j3d = np.asarray(j3d).astype(d)
        sel = np.ones(self.n, dtype=bool) if env_mask is None else np.asarray(env_mask, dtype=bool)
        with np.errstate(invalid="ignore", divide="ignore"):
            for e in np.nonzero(sel)[0]:
                p = j3d[e][self.joint_map]
                self.raw[e] = p
                trans = p[0].copy()
                p = p - trans
                scale = d.type(0)
                for i in range(1, LIMBS + 1):
                    v = p[self.parents[i]] - p[i]
                    ratio = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) / self.mean[i - 1]
                    scale = ratio if i == 1 else scale + ratio
                scale = scale / d.type(LIMBS)
                p = p / scale
                c = int(self.count[e])
                w, length = c % self.h, min(c + 1, self.h)
                self.root_ring[e, w] = trans
                self.body_ring[e, w] = p
                trans_f = self._filter(self.root_ring[e], e, w, length, np.array([1, 1, 0]))
                p_f = self._filter(self.body_ring[e], e, w, length, np.array([2, 2, 2]))
                x = p_f + trans_f
                m = self.frame
                pos = np.stack([m[i, 0] * x[:, 0] + m[i, 1] * x[:, 1] + m[i, 2] * x[:, 2] for i in range(3)], axis=-1)
                self.vel[e] = (pos - self.prev_pos[e]) / self.dt
                self.pos[e] = pos
                self.prev_pos[e] = pos
                self.count[e] = c + 1
        return self.pos, self.vel

    def state(self):
        return {"root_ring": self.root_ring.copy(), "body_ring": self.body_ring.copy(), "count": self.count.copy(), "prev_pos": self.prev_pos.copy(),
                "pos": self.pos.copy(), "vel": self.vel.copy(), "raw": self.raw.copy()}


def run(frames, history, dtype, **kw):
    """(T, N, J, 3) frames through a fresh stream -> pos, vel (T, N, J, 3) in ``dtype``."""
    frames = np.asarray(frames)
    m = StreamModel(frames.shape[1], history=history, dtype=dtype, **kw)
    pos, vel = [], []
    for f in frames:
        p, v = m.push(f)
        pos.append(p.copy())
        vel.append(v.copy())
    return np.stack(pos), np.stack(vel)
