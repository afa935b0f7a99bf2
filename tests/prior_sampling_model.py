"""Plain-torch restatement of generation from the PULSE prior (test infrastructure: never imported by pulse_amd).

AMPZBuilder.Network.form_embedding under ``flags.debug`` (phc/learning/amp_network_z_builder.py:101-119) overwrites the posterior's latent:

  a learned or fixed prior   z = reparameterize(prior_mu, prior_logvar) = prior_mu + eps * exp(0.5 prior_logvar)    :112, 245-248
                             with (prior_mu, prior_logvar) as compute_prior returns them                             :226-241
  no prior                   z = randn_like(vae_mu)                                                                  :116
  then, as always            z = project_to_norm(z, embedding_norm) under use_vae_sphere_posterior                   :118-119

and, commented out beside the live statement, the variants  z = prior_mu  (:109) and a constant log-variance of -2.3 / -1.5 in place of
prior_logvar (:110-111).  The same operations in the same order; the noise is an argument.  tests/test_prior_sampling_cpu.py holds the live
branches to the reference's own method body through tests/golden/prior_sampling.npz; the commented variants have no reference statement that
runs, so for them this file is the yardstick.
"""
import torch

from vae_variants_model import project_to_norm


def z_from_prior_heads(prior_mu, prior_logvar, eps, *, prior, clamp=True, clamp_max=2.0, fixed_logvar=0.0, sphere_prior=False, sphere_posterior=False,
                       embedding_norm=1.0, logvar_override=None):
    """``prior``: 'learned' (prior_mu, prior_logvar = the raw heads), 'fixed' (prior_mu = the raw mean head, prior_logvar ignored) or 'none'
    (both ignored).  ``eps`` None: z = the prior's mean.  ``logvar_override``: the constant that replaces the prior's log-variance."""
    if prior == "none":
        z = eps.clone()                                                                 # :116
    else:
        if prior == "learned":                                                          # compute_prior, :232-236
            if clamp:
                prior_logvar = torch.clamp(prior_logvar, min=-5, max=clamp_max)
        else:                                                                           # :237-241
            if sphere_prior:
                prior_mu = project_to_norm(prior_mu, embedding_norm)
            prior_logvar = torch.ones_like(prior_mu) * fixed_logvar
        if logvar_override is not None:                                                 # :110-111
            prior_logvar = torch.ones_like(prior_logvar) * logvar_override
        if eps is None:                                                                 # :109
            z = prior_mu
        else:                                                                           # reparameterize, :245-248
            std = torch.exp(0.5 * prior_logvar)
            z = prior_mu + eps * std
    if sphere_posterior:                                                                # :118-119
        z = project_to_norm(z, embedding_norm)
    return z


def raw_prior_heads(net, obs):
    """(prior_mu, prior_logvar) before compute_prior's clamp / projection; (None, None) without a prior, logvar None under a fixed prior."""
    if not net.has_prior:
        return None, None
    lat = net.z_prior(obs[:, :net.self_obs_size])
    return net.z_prior_mu(lat), (net.z_prior_logvar(lat) if net.use_vae_prior else None)


def net_modes(net):
    """The keywords of z_from_prior_heads that a vae_variants_model.VariantNetZ fixes."""
    return dict(prior="learned" if net.use_vae_prior else "fixed" if net.use_vae_fixed_prior else "none", clamp=net.use_vae_clamped_prior,
                clamp_max=net.var_clamp_max, fixed_logvar=net.vae_prior_fixed_logvar, sphere_prior=net.use_vae_sphere_prior,
                sphere_posterior=net.use_vae_sphere_posterior, embedding_norm=net.embedding_norm)


def prior_z(net, obs, eps, logvar_override=None):
    """The latent form_embedding leaves under flags.debug for the observation rows ``obs``."""
    mu, lv = raw_prior_heads(net, obs)
    return z_from_prior_heads(mu, lv, eps, logvar_override=logvar_override, **net_modes(net))


def generate_mu(net, obs, eps, logvar_override=None):
    """eval_actor's mean (:422-467) with that latent: the decoder on cat(self_obs, z)."""
    z = prior_z(net, obs, eps, logvar_override)
    return net.mu(net.actor_mlp(torch.cat([obs[:, :net.self_obs_size], z], dim=-1))), z
