"""Batch bookkeeping of the evaluation sweep: IMAmpAgent._post_step_eval (phc/learning/im_amp.py:244-363) without the env.

The reference walks the data set in batches of ``num_envs`` clips (HumanoidIm.begin_seq_motion_samples / forward_motion_samples) and
decides after every control step whether the batch is over.  ``EvalSweep`` is that rule, statement for statement, as torch ops on
(N,) tensors of whatever device they live on (none is needed: the CPU test runs it beside the reference's own method body), with one
small read-back per step -- the reference syncs every step as well (``.sum() > 0``, ``.max()``).  What the reference keeps as lists of
per-step position arrays is here the (N, 8) accumulator rows of pulse_im_eval_accum, collected once per batch.
"""
import math

import torch

EVAL_INFO_KEYS = ("eval_success_rate", "eval_mpjpe_all", "eval_mpjpe_succ", "accel_dist", "vel_dist", "mpjpel_all", "mpjpel_succ", "mpjpe_pa")


class EvalSweep:
    def __init__(self, num_envs, num_unique_motions, max_steps=None):
        self.num_envs, self.num_unique_motions = int(num_envs), int(num_unique_motions)
        self.max_steps = None if max_steps is None else int(max_steps)
        self.curr_steps = 0
        self.terminate_state = None
        self.terminate_memory = []                 # one (N,) bool CPU tensor per finished batch
        self.accum_memory = []                     # one (N, 8) float64 CPU tensor per finished batch
        self.batch_lengths = []                    # control steps each batch ran
        self.success_rate = 0.0

    def post_step(self, terminate, num_steps, curr_motion_ids, start_idx):
        """After a control step.  ``terminate``: the step's extras['terminate'] (N,); ``num_steps``: get_motion_num_steps() of the resident
        clips (N,); ``curr_motion_ids``: their data-set ids (N,); ``start_idx``: the env's sweep position.  Returns (batch_end, end): the
        batch is over (call ``end_batch`` with the accumulator rows, then forward_motion_samples unless ``end``) / the sweep is over."""
        n = self.num_envs
        if self.terminate_state is None:
            self.terminate_state = torch.zeros(n, dtype=torch.bool, device=terminate.device)
        num_steps = num_steps.to(torch.int64)
        # a termination after the clip's last frame is none; curr_steps is one step behind the simulation (:249-251)
        termination_state = (self.curr_steps <= num_steps - 1) & (terminate > 0)
        self.terminate_state = termination_state | self.terminate_state
        alive = ~self.terminate_state
        is_last = curr_motion_ids == self.num_unique_motions - 1
        bound = torch.argmax(is_last.to(torch.int64)) + 1                     # .nonzero()[0] + 1: behind the FIRST env that plays the last clip
        alive_b = alive & (torch.arange(n, device=alive.device) < bound)
        lowest = torch.full_like(num_steps, -1)
        flags = torch.stack([alive.any().to(torch.int64), is_last.any().to(torch.int64), alive_b.any().to(torch.int64),
                             torch.where(alive_b, num_steps, lowest).max(), torch.where(alive, num_steps, lowest).max(), num_steps.max(),
                             self.terminate_state.sum()]).tolist()            # the step's one read-back
        any_alive, has_last, any_alive_b, max_b, max_alive, max_all, num_term = flags
        if any_alive:                                                         # :252-268
            if has_last:
                curr_max = max_b if any_alive_b else self.curr_steps - 1      # the ones that should be counted have terminated
            else:
                curr_max = max_alive
            if self.curr_steps >= curr_max:
                curr_max = self.curr_steps + 1
        else:
            curr_max = max_all
        self.curr_steps += 1
        capped = self.max_steps is not None and self.curr_steps >= self.max_steps
        if not (self.curr_steps >= curr_max or num_term == n or capped):
            return False, False
        self.batch_lengths.append(self.curr_steps)
        self.curr_steps = 0
        self.terminate_memory.append(self.terminate_state.cpu())
        self.success_rate = 1.0 - float(self.terminate_history().double().mean())
        self.terminate_state = None
        return True, start_idx + n >= self.num_unique_motions

    def end_batch(self, accum):
        """The batch's accumulator rows (N, 8), copied to the host."""
        self.accum_memory.append(accum.detach().to("cpu", torch.float64).clone())

    def terminate_history(self):
        """np.concatenate(terminate_memory)[:num_unique_motions] (:278, 297-298): the wrapped tail of the last batch is cut off."""
        return torch.cat(self.terminate_memory)[:self.num_unique_motions]

    def keys(self, motion_data_keys):
        """(failed_keys, success_keys) (:310-311), in data-set order."""
        hist = self.terminate_history().tolist()
        return ([k for k, t in zip(motion_data_keys, hist) if t], [k for k, t in zip(motion_data_keys, hist) if not t])

    def eval_info(self):
        """The reference's eight numbers (:332-341).  compute_metrics_lite concatenates the frames of the motions it is given and the
        caller takes the mean: the frame-weighted mean, sum of sums / sum of counts; "succ" falls back to "all" when nothing succeeded."""
        acc = torch.cat(self.accum_memory)[:self.num_unique_motions]
        failed = self.terminate_history()
        all_ = _means(acc)
        succ = _means(acc[~failed]) if bool((~failed).any()) else all_
        return {"eval_success_rate": self.success_rate, "eval_mpjpe_all": all_["mpjpe_g"], "eval_mpjpe_succ": succ["mpjpe_g"],
                "accel_dist": succ["accel_dist"], "vel_dist": succ["vel_dist"], "mpjpel_all": all_["mpjpe_l"], "mpjpel_succ": succ["mpjpe_l"],
                "mpjpe_pa": succ["mpjpe_pa"]}


def _means(rows):
    s = rows.sum(dim=0).tolist()
    div = lambda a, c: a / c if c > 0 else math.nan            # (the mean of no frames, as numpy's)
    return {"mpjpe_g": div(s[0], s[5]), "mpjpe_l": div(s[1], s[5]), "mpjpe_pa": div(s[2], s[5]), "vel_dist": div(s[3], s[6]),
            "accel_dist": div(s[4], s[7])}
