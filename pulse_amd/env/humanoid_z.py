"""HumanoidZ on MI355X: the frozen PULSE prior + decoder INSIDE ``env.step`` (downstream-task mode).

Mirrors phc/env/tasks/humanoid_z.py:
  initialize_z_models   :24-67   load decoder / prior / running stats from a PULSE checkpoint
                                  (phc/learning/network_loader.py:139-176 reads them by key prefix; the
                                  checkpoint produced by pulse_amd's AMPZNetwork.state_dict() uses the same keys)
  compute_z_actions     :81-155  self_obs = (obs[:, :358] - mean) / sqrt(var + 1e-5)   [NOT clamped for the prior]
                                  z = z_prior_mu(z_prior(self_obs)) + action_z           [use_vae_prior only: not under a fixed prior]
                                  z = project_to_norm(z, 1, "sphere")                    [use_vae_sphere_posterior: radius 1, :106-107]
                                  action = decoder(cat(clamp(self_obs, +-5), z))
  step_z                :157-177 latent action -> PD action -> the ordinary step phases
Both MLPs run as forward launch plans of the fp32 MFMA GEMM (network_z.AMPZNetwork "prior" and "dec" plans);
the two normalisations are the pulse_rms_normalize kernel (clip = inf for the prior input, 5 for the decoder).
"""
import torch

from .. import kernels as K
from ..learning.network_z import AMPZNetwork
from .humanoid_im import HumanoidIm


class HumanoidZ:
    def _read_z_options(self, env):
        """The switches humanoid_z.py:44-48 reads from cfg['env'] about the frozen model's latent; they are the defaults of the
        task_obs_size_detail the frozen network is built from.  (use_vae_prior absent: True as before, unless the dict names the fixed
        prior, then the reference's default False.)"""
        self._z_detail = {k: env[k] for k in ("embedding_norm", "use_vae_prior", "use_vae_fixed_prior", "use_vae_sphere_prior",
                                              "use_vae_sphere_posterior", "vae_prior_fixed_logvar") if k in env}
        if "use_vae_fixed_prior" in env:
            self._z_detail.setdefault("use_vae_prior", False)

    def initialize_z_models(self, checkpoint, net_params, task_obs_size_detail=None):
        """checkpoint: {'model': state_dict with reference key names, 'running_mean_std': {...}}."""
        detail = {"embedding_size": self._embedding_size, "z_type": "vae", "use_vae_prior": True, "use_vae_clamped_prior": True,
                  "vae_var_clamp_max": 2}
        detail.update(getattr(self, "_z_detail", {}))
        detail.update(task_obs_size_detail or {})
        self._z_net = AMPZNetwork(net_params, actions_num=self._dof_size, self_obs_size=self.get_self_obs_size(),
                                  task_obs_size=detail.get("distill_task_obs_size", 576), task_obs_size_detail=detail, device=self.device)
        self._z_net.load_state_dict(checkpoint["model"])
        rms = checkpoint["running_mean_std"]
        self.running_mean = rms["running_mean"].to(self.device, torch.float64).contiguous()
        self.running_var = rms["running_var"].to(self.device, torch.float64).contiguous()
        self._z_graph = self._z_net.graph(self.num_envs)

    def compute_z_actions(self, action_z):
        net, G = self._z_net, self._z_graph
        g = G["g"]
        n, s, zc, e = self.num_envs, self.get_self_obs_size(), net.z_col, net.embedding_size
        obs = self._obs_store
        ain = g.act_bufs["ain"]
        # the prior's mean is added ``if self.use_vae_prior`` (:101-104): under a fixed prior it is NOT, and without one there is no plan
        prior_mu = None
        if net.prior_mode == K.PRIOR_LEARNED:
            # prior input: normalised, unclamped self observation (humanoid_z.py:87)
            K.rms_normalize(obs, self.running_mean, self.running_var, rows=n, cols=s, x_stride=obs.stride(0), y=G["x"], y_stride=G["x"].stride(0),
                            y_cols=s, clip=3.0e38)
            G["fwd_prior"].run()
            prior_mu = g.act_bufs["pheads"][:, :e]
        # decoder input: clamp(self_obs, +-5) (:149) | z = prior_mu + action_z (:102-103); project_to_norm(.., "none") is a no-op
        K.rms_normalize(obs, self.running_mean, self.running_var, rows=n, cols=s, x_stride=obs.stride(0), y=ain, y_stride=ain.stride(0),
                        y_cols=s, clip=5.0)
        z = ain[:, zc:zc + e]
        if net.use_vae_sphere_posterior:
            # project_to_norm(action_z, 1, "sphere") (:106-107): radius 1 whatever embedding_norm the model trained with -- the
            # reference's own mismatch, kept
            K.vae_project(action_z, z, rows=n, cols=e, norm=1.0, b=prior_mu)
        elif prior_mu is not None:
            torch.add(prior_mu, action_z, out=z)
        else:
            z.copy_(action_z)
        G["fwd_dec"].run()
        return g.act_bufs["mu"][:, :self._dof_size]

    def set_action_clip(self, clip):
        """The wrapper's clip_actions bounds what step() takes, the latent: the decoded PD action is not clamped (the reference's wrapper never
        sees it), so the clamp stays in the wrapper."""
        return False

    def step_z(self, action_z):
        self.action_z = action_z
        actions = self.compute_z_actions(action_z)
        self.pre_physics_step(actions)
        self._physics_step()
        self.post_physics_step()


class HumanoidImZ(HumanoidIm, HumanoidZ):
    """HumanoidImZ (phc/env/tasks/humanoid_im.py:1199-1214): imitation task whose action is the 32-d latent."""

    def __init__(self, cfg, sim, motion_lib, device="cuda:0"):
        super().__init__(cfg, sim, motion_lib, device=device)
        env = cfg.get("env", cfg)
        self._embedding_size = int(env.get("embedding_size", 32))
        self.num_actions = self._embedding_size                                # _setup_character_props_z (:65-67)
        self._read_z_options(env)

    set_action_clip = HumanoidZ.set_action_clip

    def step(self, action_z):
        self.step_z(action_z)
