"""The op-by-op sequence of play_steps (amp_agent.py:372-412) with rl_games' AverageMeter on the CPU: the reference that the
pulse_rollout_record tests compare the one-launch kernel with (test_learner_kernels_gpu.py, test_small_kernel_branches_gpu.py)."""
import numpy as np
import torch


class RolloutReference:
    """Episode accumulators and the two AverageMeters, ``[mean, size]`` each, advanced one rollout step at a time."""

    def __init__(self, cur_r, cur_l, meter_r, meter_l, max_size, value_mean=None, value_var=None, value_eps=1e-5):
        self.cur_r, self.cur_l = cur_r.clone(), cur_l.clone()
        self.meter_r, self.meter_l = [float(x) for x in meter_r], [float(x) for x in meter_l]
        self.max_size = max_size
        self.vmean, self.vvar, self.veps = value_mean, value_var, value_eps

    def step(self, rew, dones, term, value_raw=None):
        """One step on CPU tensors (rew float (n,), dones / term int (n,), value_raw (n,) or None).  Returns the bootstrap values written
        to the buffer (None without value_raw); the accumulators and meters are updated in place."""
        nv = None
        if value_raw is not None:
            v = value_raw
            if self.vmean is not None:
                v = torch.sqrt(self.vvar.float() + self.veps) * torch.clamp(v, -5, 5) + self.vmean.float()
            nv = v * (1.0 - term.float())
        self.cur_r = self.cur_r + rew
        self.cur_l = self.cur_l + 1
        idx = dones.nonzero().flatten()
        for st, vals in ((self.meter_r, self.cur_r[idx]), (self.meter_l, self.cur_l[idx])):
            size = vals.shape[0]
            if size == 0:
                continue
            new_mean = vals.float().mean().item()
            size = float(np.clip(size, 0, self.max_size))
            old = min(self.max_size - size, st[1])
            st[0], st[1] = (st[0] * old + new_mean * size) / (old + size), old + size
        nd = 1.0 - dones.float()
        self.cur_r, self.cur_l = self.cur_r * nd, self.cur_l * nd
        return nv
