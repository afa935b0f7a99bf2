"""Plain-torch restatement of the PULSE VAE's prior / posterior variants (test infrastructure: never imported by pulse_amd).

The four switches of AMPZBuilder.Network (phc/learning/amp_network_z_builder.py:40-46) on top of oracle.agent_oracle.OracleNetZ, with the
same operations in the same order as the reference:

  form_embedding      :79-121    clamp, re-parameterisation, ``flags.test`` replacement z = mu, THEN the sphere posterior; the extra dict
                                 keeps the unprojected heads
  compute_prior       :226-241   learned (if) / fixed with an optional sphere projection of the mean (elif) / nothing
  optimize_kin        phc/learning/amp_agent.py:771-849   kl_multi against a learned or fixed prior, the N(0, I) form without one
  compute_z_actions   phc/env/tasks/humanoid_z.py:81-155  prior mean added only ``if use_vae_prior``; sphere posterior with radius 1

Parameters a mode does not have are dropped (no z_prior_logvar under a fixed prior, no z_prior* without a prior), as :514-533 builds them.
tests/test_vae_variants_cpu.py holds this file to the reference's own method bodies through tests/golden/vae_variants.npz.
"""
import torch

from oracle import agent_oracle as AO

MODES = {          # name -> the switches as an env dict spells them
    "learned": dict(use_vae_prior=True, use_vae_fixed_prior=False, use_vae_sphere_prior=False),
    "fixed": dict(use_vae_prior=False, use_vae_fixed_prior=True, use_vae_sphere_prior=False),
    "fixed_sphere": dict(use_vae_prior=False, use_vae_fixed_prior=True, use_vae_sphere_prior=True),
    "none": dict(use_vae_prior=False, use_vae_fixed_prior=False, use_vae_sphere_prior=False),
}


def project_to_norm(x, norm):
    """phc/utils/torch_utils.py:38-43, z_type 'sphere'."""
    return x / (torch.norm(x, dim=-1, keepdim=True) / norm + 1e-8)


class VariantNetZ(AO.OracleNetZ):
    def __init__(self, *, use_vae_prior=True, use_vae_fixed_prior=False, use_vae_sphere_prior=False, use_vae_sphere_posterior=False,
                 vae_prior_fixed_logvar=0.0, embedding_norm=1.0, use_vae_clamped_prior=True, **kw):
        super().__init__(**kw)                                  # (draws every parameter of the learned form, then drops: same draws per mode)
        self.use_vae_prior, self.use_vae_fixed_prior = bool(use_vae_prior), bool(use_vae_fixed_prior)
        self.use_vae_sphere_prior, self.use_vae_sphere_posterior = bool(use_vae_sphere_prior), bool(use_vae_sphere_posterior)
        self.vae_prior_fixed_logvar, self.embedding_norm = vae_prior_fixed_logvar, embedding_norm
        self.use_vae_clamped_prior = bool(use_vae_clamped_prior)
        self.test = False                                       # flags.test
        if not self.use_vae_prior:                              # :514-533
            del self.z_prior_logvar
            if not self.use_vae_fixed_prior:
                del self.z_prior, self.z_prior_mu

    @property
    def has_prior(self):
        return self.use_vae_prior or self.use_vae_fixed_prior

    def form_embedding(self, task_out_z, noise):
        vae_mu = self.z_mu(task_out_z)
        vae_log_var = self.z_logvar(task_out_z)
        if self.use_vae_clamped_prior:
            vae_log_var = torch.clamp(vae_log_var, min=-5, max=self.var_clamp_max)
        z = vae_mu + torch.exp(0.5 * vae_log_var) * noise
        if self.test:
            z = vae_mu
        if self.use_vae_sphere_posterior:
            z = project_to_norm(z, self.embedding_norm)
        return z, {"vae_mu": vae_mu, "vae_log_var": vae_log_var, "noise": noise}

    def compute_prior(self, obs):
        lat = self.z_prior(obs[:, :self.self_obs_size])
        prior_mu = self.z_prior_mu(lat)
        if self.use_vae_prior:
            prior_logvar = self.z_prior_logvar(lat)
            if self.use_vae_clamped_prior:
                prior_logvar = torch.clamp(prior_logvar, min=-5, max=self.var_clamp_max)
            return prior_mu, prior_logvar
        elif self.use_vae_fixed_prior:
            if self.use_vae_sphere_prior:
                return project_to_norm(prior_mu, self.embedding_norm), torch.ones_like(prior_mu) * self.vae_prior_fixed_logvar
            return prior_mu, torch.ones_like(prior_mu) * self.vae_prior_fixed_logvar


def optimize_kin(net, obs, gt_action, progress_buf, noise, horizon, kld_coefficient=0.01, ar1_coefficient=0.005, use_ar1_prior=True,
                 use_vae_prior_regu=False):
    """AMPAgent._optimize_kin (amp_agent.py:771-849) up to and including kin_loss.backward(); gradients are left in ``net``."""
    mb = obs.shape[0]
    pred_action, _, extra = net.eval_actor(obs, noise)
    kin_action_loss = torch.norm(pred_action - gt_action, dim=-1).mean()
    vae_mu, vae_log_var = extra["vae_mu"], extra["vae_log_var"]
    if net.has_prior:
        prior_mu, prior_log_var = net.compute_prior(obs)
        KLD = AO.kl_multi(vae_mu, vae_log_var, prior_mu, prior_log_var).mean()
    else:
        KLD = -0.5 * torch.sum(1 + vae_log_var - vae_mu.pow(2) - vae_log_var.exp()) / vae_mu.shape[0]
    ar1_prior, regu_prior = 0, 0
    info = {}
    if use_ar1_prior:
        time_zs = vae_mu.view(mb // horizon, horizon, -1)
        phi = 0.99
        error = time_zs[:, 1:] - time_zs[:, :-1] * phi
        idxes = progress_buf.view(mb // horizon, horizon, -1)
        not_consecs = ((idxes[:, 1:] - idxes[:, :-1]) != 1).view(-1)
        error = error.reshape(-1, error.shape[-1]).clone()
        error[not_consecs] = 0
        starteres = ((idxes <= 2)[:, 1:] + (idxes <= 2)[:, :-1]).view(-1)
        error[starteres] = 0
        ar1_prior = torch.norm(error, dim=-1).mean()
        info["kin_ar1"] = ar1_prior.detach()
    if use_vae_prior_regu:
        prior_mean_regu = ((prior_mu ** 2).mean() + (vae_mu ** 2).mean()) * 0.001
        prior_var_regu = ((prior_log_var ** 2).mean() + (vae_log_var ** 2).mean()) * 0.001
        regu_prior = prior_mean_regu + prior_var_regu
        info["kin_prior_regu"] = regu_prior.detach()
    kin_loss = kin_action_loss + KLD * kld_coefficient + ar1_prior * ar1_coefficient + regu_prior * 0.005
    for p in net.parameters():
        p.grad = None
    kin_loss.backward()
    info.update({"kin_action_loss": kin_action_loss.detach(), "kin_KLD": KLD.detach(), "kin_loss": kin_loss.detach()})
    return info


def compute_z_actions(net, obs_buf, running_mean, running_var, action_z):
    """HumanoidZ.compute_z_actions (humanoid_z.py:81-155), z_type 'vae', not z_all."""
    with torch.no_grad():
        s = net.self_obs_size
        self_obs = (obs_buf[:, :s] - running_mean.float()[:s]) / torch.sqrt(running_var.float()[:s] + 1e-05)
        if net.use_vae_prior:
            action_z = net.z_prior_mu(net.z_prior(self_obs)) + action_z
        if net.use_vae_sphere_posterior:
            action_z = project_to_norm(action_z, 1)
        self_obs = torch.clamp(self_obs, min=-5.0, max=5.0)
        return net.mu(net.actor_mlp(torch.cat([self_obs, action_z], dim=-1)))
