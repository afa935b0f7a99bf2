"""IMAmpAgent: the registered algo name ``im_amp`` (phc/run_hydra.py:266) of every imitation config.

Mirrors phc/learning/im_amp.py:39-132 on top of AMPAgent:
  get_action            :44-76   deterministic / sampled action for evaluation loops
  env_eval_step         :78-100
  restore               :102-118 checkpoint + the newest termination history (failed_*.pkl) pushed into the motion library's
                                 sampling probabilities
  update_training_data  :127-132 PMCP: hard / soft re-weighting of the motion sampling from the keys that failed evaluation
  eval                  :136-363 the sweep over the whole motion data set in batches of num_envs clips under evaluation rules
                                 (HumanoidIm.evaluation_mode), with _post_step_eval's batch bookkeeping (learning/eval_sweep.py).  The
                                 reference copies every step's body positions to the host and computes smpl_sim's compute_metrics_lite
                                 (a third-party dependency that is absent) at the end; here pulse_im_eval_accum sums the same five
                                 per-frame terms on the device (include/pulse_hip.h 2b'' fixes their definitions).  failed_keys are
                                 motion keys, what update_hard / soft_sampling_weight index the data set by.
"""
import glob
import os
import os.path as osp
import pickle

import torch

from .amp_agent import AMPAgent


class IMAmpAgent(AMPAgent):
    def __init__(self, base_name, config):
        super().__init__(base_name, config)
        self.network_path = config.get("network_path", osp.join(config.get("train_dir", "output/pulse_amd"), "nn"))
        self.has_batch_dimension = True
        self.is_tensor_obses = True

    # ------------------------------------------------------------------ im_amp.py:44-76
    def get_action(self, obs_dict, is_determenistic=False):
        obs = obs_dict["obs"] if isinstance(obs_dict, dict) else obs_dict
        n = obs.shape[0]
        net = self.model
        ws = net.workspace(n, train=False)
        net.eval()
        self.running_mean_std.eval()
        self._preproc_obs(self._obs_store(obs), ws, n)
        net.forward(ws, n)
        mu = ws["mu"]
        if is_determenistic:
            current_action = mu.clone()
        else:
            noise = torch.randn(n, self.actions_num, device=self.ppo_device, generator=self.noise_generator)
            current_action = mu + torch.exp(net.sigma) * noise
        if self.clip_actions:
            d, m = (self.actions_high - self.actions_low) / 2.0, (self.actions_high + self.actions_low) / 2.0
            return torch.clamp(current_action, -1.0, 1.0) * d + m                 # rescale_actions
        return current_action

    def env_eval_step(self, env, actions):
        obs, rewards, dones, infos = env.step(actions)
        return obs, rewards.to(self.ppo_device), dones.to(self.ppo_device), infos

    # ------------------------------------------------------------------ im_amp.py:102-132
    def restore(self, fn):
        super().restore(fn)
        fails = glob.glob(osp.join(self.network_path, "failed_*"))
        if fails:
            newest = sorted(fails, key=lambda x: int(x.split("_")[-1].split(".")[0]))[-1]
            with open(newest, "rb") as f:
                history = pickle.load(f)["termination_history"]
            self.vec_env.env.task._motion_lib.update_sampling_prob(history)

    def update_training_data(self, failed_keys):
        task = self.vec_env.env.task
        lib = task._motion_lib
        # (no hasattr guards: a motion source without the PMCP hooks fails loudly instead of silently training on the old weights)
        if task.auto_pmcp:
            lib.update_hard_sampling_weight(failed_keys)
        elif task.auto_pmcp_soft:
            lib.update_soft_sampling_weight(failed_keys)
        os.makedirs(self.network_path, exist_ok=True)
        with open(osp.join(self.network_path, f"failed_{self.epoch_num:010d}.pkl"), "wb") as f:
            pickle.dump({"failed_keys": failed_keys, "termination_history": lib._termination_history}, f)

    # ------------------------------------------------------------------ im_amp.py:136-363
    def eval(self, max_steps=None, return_positions=False):
        """The reference's evaluation sweep: the whole data set in batches of num_envs clips under evaluation rules (HumanoidIm.evaluation_mode),
        deterministic actions, batch bookkeeping by EvalSweep (_post_step_eval), metrics summed on the device by pulse_im_eval_accum.  Ends
        with update_training_data(failed_keys) -- motion keys -- and the env back in training mode, every env reset.  ``max_steps`` caps a
        batch.  The env must take its reference from a MotionLib (recorded reference frames have no data set to walk: evaluation_mode raises).
        ``return_positions``: also copy every step's positions out and return per-motion (T_i, J, 3) pred / gt arrays (the
        reference's pred_pos_all / gt_pos_all; tests and debugging)."""
        from .eval_sweep import EvalSweep
        task = self.vec_env.env.task
        n = task.num_envs
        max_steps = int(max_steps or task.max_episode_length)
        self.set_eval()
        positions = {"pred": [], "gt": []}
        with torch.no_grad(), task.evaluation_mode(record_positions=return_positions) as st:
            lib = task._motion_lib
            sweep = EvalSweep(n, lib._num_unique_motions, max_steps=max_steps)
            task.begin_seq_motion_samples()
            obs = task.obs_buf
            while True:
                act = self.get_action({"obs": obs}, is_determenistic=True)
                obs, _, dones, infos = self.env_eval_step(self.vec_env, act)
                batch_end, end = sweep.post_step(infos["terminate"], st["num_steps"], task.eval_curr_motion_ids(), task.start_idx)
                if batch_end:
                    sweep.end_batch(st["accum"])
                    if return_positions:
                        self._slice_positions(st["record"], st["num_steps"].tolist(), positions)
                        st["record"].clear()
                    if end:
                        break
                    task.forward_motion_samples()          # done[:] = 1: the next batch of clips, every env reset
                    obs = task.obs_buf
                else:
                    obs = self.vec_env.reset_masked(dones > 0)
            keys = lib._motion_data_keys
            failed_keys, success_keys = sweep.keys(keys)
            info = sweep.eval_info()
            num_motions = lib._num_unique_motions
        self.vec_env.reset()                               # every env, back in training mode (:234)
        self.update_training_data(failed_keys)
        out = dict(info)
        out.update({"success_rate": info["eval_success_rate"], "mpjpe_g": info["eval_mpjpe_all"], "mpjpe_l": info["mpjpel_all"],
                    "failed_keys": failed_keys, "success_keys": success_keys, "num_motions": num_motions, "motion_keys": list(keys),
                    "batch_lengths": list(sweep.batch_lengths)})
        if return_positions:
            out["pred_pos_all"], out["gt_pos_all"] = positions["pred"][:num_motions], positions["gt"][:num_motions]
        return out

    @staticmethod
    def _slice_positions(record, num_steps, positions):
        """all_body_pos_pred[:(i - 1), idx] (im_amp.py:284-287): motion idx keeps the first num_steps - 1 recorded steps of its batch."""
        import numpy as np
        pred, gt = np.stack([r[0] for r in record]), np.stack([r[1] for r in record])
        for idx, i in enumerate(num_steps):
            positions["pred"].append(pred[:max(i - 1, 0), idx])
            positions["gt"].append(gt[:max(i - 1, 0), idx])
