"""Players: load a checkpoint and act, without a learner.

Mirrors rl_games' BasePlayer / phc/learning/common_player.py:35-175 (run loop) and phc/learning/amp_players.py:16-110
(AMPPlayerContinuous: restore also loads ``amp_input_mean_std``; discriminator reward for debugging, :112-160).
The networks are the same GEMM launch plans the agents use; the checkpoint layout is the reference's ({'model', 'running_mean_std',
'reward_mean_std', 'amp_input_mean_std'}, phc/learning/network_loader.py wire format).
"""
import torch

from .common_agent import CommonAgent
from .amp_agent import AMPAgent


def check_z_source_options(config, detail=None):
    """config['player']['z_source'] / ['prior_logvar'] -> (z_source, prior_logvar), validated without a device.  ``detail``: the env's
    task_obs_size_detail (the prior switches); default: read off config['vec_env'] when the env is already there, otherwise only what needs no
    env is checked here and the model's own setter checks the rest once it exists."""
    from .network_z import check_z_source, prior_mode_of
    p = config.get("player", {}) or {}
    z_source, prior_logvar = p.get("z_source", "posterior"), p.get("prior_logvar", None)
    check_z_source(z_source, prior_logvar, None)
    if z_source == "posterior":
        return z_source, prior_logvar
    name = config["network"].get("name", "amp")
    if name != "amp_z":
        raise ValueError(f"player z_source {z_source!r} on network {name!r}: only amp_z has a latent with a prior to draw from "
                         "(amp_network_z_builder.py:101-116)")
    if detail is None and "vec_env" in config:
        detail = config["vec_env"].env.task.get_task_obs_size_detail()
    if detail is not None:
        check_z_source(z_source, prior_logvar, prior_mode_of(detail))
    return z_source, prior_logvar


class CommonPlayer:
    AGENT = CommonAgent

    def __init__(self, config):
        self.config = config
        self.z_source, self.prior_logvar = check_z_source_options(config)      # before any device work
        # a player is an agent that never trains: construction builds the networks, normalisers and env plumbing once
        self._agent = self.AGENT("player", config)
        a = self._agent
        if self.z_source != "posterior":
            a.model.set_z_source(self.z_source, self.prior_logvar)
        self.env, self.device = a.vec_env, a.ppo_device
        self.model, self.running_mean_std = a.model, a.running_mean_std
        self.actions_num, self.clip_actions = a.actions_num, a.clip_actions
        self.games_num = int(config.get("player", {}).get("games_num", 2000))
        self.is_determenistic = bool(config.get("player", {}).get("determenistic", True))
        self.max_steps = int(config.get("player", {}).get("max_steps", 108000))

    def restore(self, fn):
        ckpt = torch.load(fn, map_location=self.device, weights_only=False) if isinstance(fn, str) else fn
        self._agent.set_full_state_weights(ckpt)
        return ckpt

    def get_action(self, obs, is_determenistic=False):
        a = self._agent
        n = obs.shape[0]
        ws = a.model.workspace(n, train=False)
        a.set_eval()
        a._preproc_obs(obs, ws, n)
        a.model.forward(ws, n)
        mu = ws["mu"]
        act = mu.clone() if is_determenistic else mu + torch.exp(a.model.sigma) * torch.randn(n, self.actions_num, device=self.device)
        return torch.clamp(act, -1.0, 1.0) if self.clip_actions else act

    def _post_step(self, info):
        return

    def run(self, n_steps=None):
        """common_player.py:35-175 reduced to its data path: step all envs, reset the finished ones, average episode returns."""
        env = self.env
        obs = env.reset()
        n = env.num_envs
        cr = torch.zeros(n, device=self.device)
        sum_rewards, games = 0.0, 0
        for _ in range(int(n_steps or self.max_steps)):
            action = self.get_action(obs, self.is_determenistic)
            obs, r, done, info = env.step(action)
            cr += r
            self._post_step(info)
            d = done > 0
            k = int(d.sum())
            if k:
                sum_rewards += float(cr[d].sum())
                games += k
                cr.mul_(~d)
                obs = env.reset_masked(d)
            if games >= self.games_num:
                break
        return {"games": games, "av_reward": sum_rewards / max(1, games)}

    def generate(self, n_steps, record=False):
        """The run loop as a motion generator: ``n_steps`` steps of every env, finished envs reset as in ``run``.  With z_source 'prior' (&c)
        the humanoid moves from the prior's samples alone.  -> {'steps', 'resets'}; ``record``: also 'rb' (T, N, J, 13), the simulator's
        rigid-body state after each step, and -- for a network with a latent -- 'z' (T, N, E), the latent of each step; both stay on the device."""
        return self._generate(n_steps, record, record)

    def generate_motion(self, n_steps, *, form="motion", min_frames=2, skeleton_trees=None, **export):
        """``generate`` with a recorder attached (env/motion_export.py): the rollout as motion clips, one per episode segment of every env, keyed
        f"{env}_{k}" -- ``MotionLib.from_motion_data`` takes the result as it is (form "motion"; ``min_frames=2`` because it rejects one-frame
        clips; the dropped segments are reported in ``.dropped``).  For a network with a latent every clip also carries "z" (F, E).  ``export``: further
        arguments of ``export_motion`` (fps, root_offset, upright_start ...).  One ``pulse_motion_export`` launch after the loop."""
        return self._motion(n_steps, None, skeleton_trees, form=form, min_frames=min_frames, **export)

    def track(self, keypoints, record=False):
        """Drive a keypoint-demo env (HumanoidImMCPDemo / HumanoidImDemo, configs "mcp_demo_small" / "im_demo_small") with streamed keypoints:
        ``keypoints`` is a (T, N, 24, 3) float32 device tensor or an iterable of (N, 24, 3) frames; per frame: ``task.push_keypoints(frame)``
        (one pulse_keypoint_push launch), ``get_action``, ``env.step``.  Returns what ``generate`` returns (the demo never resets: 'resets' is 0)."""
        return self._generate(None, record, record, frames=self._frames(keypoints))

    def track_motion(self, keypoints, *, form="motion", min_frames=2, skeleton_trees=None, **export):
        """``track`` with a recorder attached: the tracked motion as clips, one per env -- ``MotionLib.from_motion_data`` takes the result as it is
        (``generate_motion``'s arguments and layout)."""
        frames = self._frames(keypoints)
        return self._motion(len(frames), frames, skeleton_trees, form=form, min_frames=min_frames, **export)

    def _frames(self, keypoints):
        if not hasattr(self.env.task, "push_keypoints"):
            raise TypeError(f"track: {type(self.env.task).__name__} takes no keypoints (HumanoidImMCPDemo / HumanoidImDemo do: configs 'mcp_demo_small', "
                            "'im_demo_small')")
        return keypoints if isinstance(keypoints, torch.Tensor) else list(keypoints)

    def _motion(self, n_steps, frames, skeleton_trees, **export):
        from ..env.motion_export import MotionRecorder
        recorder = MotionRecorder(self.env.task, int(n_steps))
        run = self._generate(n_steps, False, True, recorder, frames=frames)
        out = recorder.export(skeleton_trees, **export)
        if "z" in run and len(out):
            z, seg = run["z"].cpu().numpy(), out.segments
            for key, e, t0, f in zip(seg["keys"], seg["env"].tolist(), seg["t0"].tolist(), seg["frames"].tolist()):
                out[key]["z"] = z[t0:t0 + f, e].copy()
        return out

    def _generate(self, n_steps, record_rb, record_z, recorder=None, frames=None):
        env, n, T = self.env, self.env.num_envs, int(n_steps if frames is None else len(frames))
        record = record_rb
        obs = env.reset()
        has_z = record_z and hasattr(self.model, "z_source")        # amp_z: the policy has a latent to record
        ws = self.model.workspace(n, train=False) if has_z else None
        out = {}
        if record:
            out["rb"] = torch.empty((T,) + tuple(env.task.sim.rigid_body_state.shape), device=self.device)
        if has_z:
            out["z"] = torch.empty(T, n, ws["z"].shape[1], device=self.device)
        resets = torch.zeros((), dtype=torch.int64, device=self.device)
        try:
            for t in range(T):
                if has_z:
                    ws["z_record"] = out["z"][t]                    # the prior launch writes the step's z there itself
                if frames is not None:
                    env.task.push_keypoints(frames[t])              # the reference of the observation this step ends with
                action = self.get_action(obs, self.is_determenistic)
                if has_z and self.model.z_source == "posterior":    # (the posterior launch has no recorder output)
                    out["z"][t].copy_(ws["z"])
                obs, _, done, info = env.step(action)
                self._post_step(info)
                if record:
                    out["rb"][t].copy_(env.task.sim.rigid_body_state)
                if recorder is not None:
                    recorder.record()
                d = done > 0
                resets += d.sum()
                obs = env.reset_masked(d)                           # (a mask, no read-back: one host sync at the end of the loop)
        finally:
            if has_z:
                ws["z_record"] = None
        out.update(steps=T, resets=int(resets))
        return out


class AMPPlayerContinuous(CommonPlayer):
    AGENT = AMPAgent

    def __init__(self, config):
        self._normalize_amp_input = config.get("normalize_amp_input", True)
        self._disc_reward_scale = config.get("disc_reward_scale", 2)
        super().__init__(config)

    def restore(self, fn):
        ckpt = super().restore(fn)                      # AMPAgent.set_full_state_weights also restores amp_input_mean_std (amp_players.py:64-73)
        return ckpt

    def _calc_disc_rewards(self, amp_obs):
        """amp_players.py:148-160 (debug read-out of the discriminator reward)."""
        a = self._agent
        if not getattr(a, "enable_disc", False):
            raise RuntimeError("this checkpoint / config has no discriminator")
        pad = torch.zeros(amp_obs.shape[0], a._amp_pitch, device=self.device)
        pad[:, :a._amp_dim] = amp_obs
        return a._calc_disc_rewards(pad)


class IMAMPPlayerContinuous(AMPPlayerContinuous):
    """phc/learning/im_amp_players.py: the player registered under ``im_amp`` -- evaluation over the motion library."""

    def __init__(self, config):
        from .im_amp import IMAmpAgent
        self.AGENT = IMAmpAgent
        super().__init__(config)

    def run(self, n_steps=None):
        return self._agent.eval(max_steps=n_steps)
