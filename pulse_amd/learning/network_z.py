"""PULSE VAE policy network (``network: amp_z``) on the gfx950 kernels.

Mirrors AMPZBuilder.Network, phc/learning/amp_network_z_builder.py (z_type "vae", non-RNN branch) with the sizes of
learning/im_z_fit.yaml + env/env_im_vae.yaml.  The prior is learned (use_vae_prior, the shipped form), fixed (use_vae_fixed_prior:
z_prior + z_prior_mu only, constant log-variance vae_prior_fixed_logvar, the mean optionally on the sphere of radius embedding_norm:
use_vae_sphere_prior) or absent (neither switch: no z_prior* parameters, KL against N(0, I)); use_vae_sphere_posterior projects z after
the re-parameterisation (:118-119).  z_all, z_readout and z_type other than "vae" raise by name.

  encoder   z_mlp: obs(934) -> [1536,1024,512] SiLU -> Linear(160)            :469-492
            z_mu / z_logvar: Linear(160 -> 32) each                          :507-511
  prior     z_prior: self_obs(358) -> [1536,1024,512] SiLU; z_prior_mu / z_prior_logvar (512 -> 32)   :513-518, 226-241
  decoder   actor_mlp: cat(self_obs, z)(390) -> [3096,2048,1024] SiLU; mu (1024 -> 69)                :422-467
  critic    critic_z_mlp: obs -> [1536,1024,512] SiLU -> Linear(32); critic_mlp: cat(self_obs, .) -> ... -> value   :559-580, 326-339

The heavy part (every Linear, forward and backward) runs as launch plans of the fp32 MFMA GEMM
(learning/graph.py).  The head-level algebra of form_embedding (:82-121: log-var clamp [-5, vae_var_clamp_max],
re-parameterisation) and of the losses is tiny ((B,32)/(B,69) tensors) and is done with ordinary
tensor ops by the caller between the plans; its gradients are fed back through ``seed_*``.

Physical layout notes: z_mu|z_logvar and (learned prior) z_prior_mu|z_prior_logvar are each ONE stacked (64, .) matrix
(one GEMM, no gradient accumulation at their shared input); cat(self_obs, z) is a 392-float buffer with
self_obs at columns 0..357 and z at 360..391 (16-byte aligned segment), the first decoder / critic layer's
weight carries the same column layout.  ``state_dict`` speaks the reference's names and shapes.
"""
import torch

from .. import kernels as K
from .._lib import ACT_NONE
from .graph import GraphNetwork, Linear, _concat_plans, r4


Z_SOURCES = ("posterior", "prior", "prior_mean", "normal")


def prior_mode_of(detail):
    """The prior an env's task_obs_size_detail asks for: learned wins when both switches are on (``if use_vae_prior / elif
    use_vae_fixed_prior``, amp_network_z_builder.py:232-241, 514-533); use_vae_prior defaults to on."""
    return K.PRIOR_LEARNED if bool(detail.get("use_vae_prior", True)) else K.PRIOR_FIXED if bool(detail.get("use_vae_fixed_prior", False)) else K.PRIOR_NONE


def check_z_source(z_source, prior_logvar, prior_mode):
    """Where the policy's latent comes from (form_embedding, amp_network_z_builder.py:79-121): 'posterior' = the encoder (training, tracking);
    under flags.debug (:101-116) 'prior' = reparameterize(prior_mu, prior_logvar), 'prior_mean' = prior_mu (:109), 'normal' = randn_like, the
    branch of a network WITHOUT a prior (:116).  ``prior_logvar``: None or the constant log-variance of :110-111.  Needs no device."""
    if z_source not in Z_SOURCES:
        raise ValueError(f"z_source {z_source!r}: one of {', '.join(Z_SOURCES)}")
    if prior_logvar is not None and (isinstance(prior_logvar, bool) or not isinstance(prior_logvar, (int, float)) or prior_logvar != prior_logvar):
        raise ValueError(f"prior_logvar {prior_logvar!r}: None or a float (the constant log-variance, amp_network_z_builder.py:110-111)")
    if prior_logvar is not None and z_source != "prior":
        raise ValueError(f"prior_logvar with z_source {z_source!r}: the constant log-variance replaces the prior's, which only 'prior' reads")
    if prior_mode is None:                                      # (the network is not known yet: the options alone)
        return
    if z_source in ("prior", "prior_mean") and prior_mode == K.PRIOR_NONE:
        raise ValueError(f"z_source {z_source!r} needs a prior: the network has neither use_vae_prior nor use_vae_fixed_prior "
                         "(z_source 'normal' is the reference's branch there, amp_network_z_builder.py:116)")
    if z_source == "normal" and prior_mode != K.PRIOR_NONE:
        raise ValueError("z_source 'normal' is the reference's branch for a network without a prior (amp_network_z_builder.py:115-116); with "
                         "use_vae_prior / use_vae_fixed_prior on it cannot be reached: use 'prior'")


class AMPZNetwork(GraphNetwork):
    def __init__(self, params, *, actions_num, self_obs_size, task_obs_size, task_obs_size_detail, device="cuda:0", split_k=8):
        d = task_obs_size_detail
        self.embedding_size = int(d.get("embedding_size", 32))
        if self.embedding_size > 32:
            raise NotImplementedError(f"amp_z with embedding_size {self.embedding_size}: the VAE head kernels map lane = latent inside 32 lanes "
                                      "(vae_head.hip: embedding_size <= 32); PULSE-X's 48 latents (env_pulsex_amp.yaml) are not built")
        self.z_type = d.get("z_type", "vae")
        if self.z_type != "vae":
            raise NotImplementedError("only z_type 'vae' (the shipped PULSE configuration) is built")
        for k, where in (("z_all", "amp_network_z_builder.py:37, 52-55 (z fed to every decoder layer)"),
                         ("z_readout", "amp_network_z_builder.py:63-64, amp_network_z_reader_builder.py:36")):
            if d.get(k, False):
                raise NotImplementedError(f"amp_z with {k}: not built; reference: phc/learning/{where}")
        # the prior: learned (state-conditioned mean and log-variance) / fixed (learned mean, constant log-variance) / none (KL against
        # N(0, I)); both places of the reference use ``if use_vae_prior / elif use_vae_fixed_prior`` (:232-241, 514-533): learned wins
        self.use_vae_prior = bool(d.get("use_vae_prior", True))
        self.use_vae_fixed_prior = bool(d.get("use_vae_fixed_prior", False))
        self.prior_mode = prior_mode_of(d)
        self.vae_prior_fixed_logvar = float(d.get("vae_prior_fixed_logvar", 0))
        # use_vae_sphere_prior acts inside the fixed-prior branch only (:237-239); with a learned prior or none it has no effect
        self.use_vae_sphere_prior = bool(d.get("use_vae_sphere_prior", False))
        self.sphere_prior = self.use_vae_sphere_prior and self.prior_mode == K.PRIOR_FIXED
        self.use_vae_sphere_posterior = bool(d.get("use_vae_sphere_posterior", False))
        self.embedding_norm = float(d.get("embedding_norm", 1))
        if (self.sphere_prior or self.use_vae_sphere_posterior) and not self.embedding_norm > 0:
            raise ValueError(f"embedding_norm {self.embedding_norm}: the sphere projections need a positive radius")
        self.use_vae_clamped_prior = bool(d.get("use_vae_clamped_prior", True))
        self.vae_var_clamp_max = float(d.get("vae_var_clamp_max", 2))
        self.units = [int(u) for u in params["mlp"]["units"]]
        self.task_units = [int(u) for u in params["task_mlp"]["units"]]
        self.act = K.ACTIVATIONS[params["mlp"]["activation"]]
        self.task_act = K.ACTIVATIONS[params["task_mlp"]["activation"]]
        S = int(self_obs_size)
        self.z_col = r4(S)                                      # 360: where z starts inside cat(self_obs, z)
        self.cat_width = self.z_col + self.embedding_size
        self.cat_map = list(range(S)) + list(range(self.z_col, self.z_col + self.embedding_size))
        super().__init__(params, actions_num=actions_num, self_obs_size=self_obs_size, task_obs_size=task_obs_size, device=device, split_k=split_k)

    # ------------------------------------------------------------------ construction
    def _build(self, m, x=None):
        E, S, T, U = self.embedding_size, self.self_obs_size, self.task_units, self.units
        g, book = self._new_graph(m, x), self.book
        g.buffer("ain", self.cat_width)
        g.buffer("cin", self.cat_width)
        lins = {}
        zc = (self.z_col, self.cat_width, ACT_NONE, None, 0)
        # A2CBuilder order: actor_mlp, critic_mlp, value, mu (network_builder.py:245-261)
        lins["actor_mlp"] = g.mlp("a2c_network.actor_mlp", "ain", S + E, U, self.act, ["a1", "a2", "a3"][:len(U)], colmap=self.cat_map,
                                  first_grad_ranges=[zc], tag="dec")
        lins["critic_mlp"] = g.mlp("a2c_network.critic_mlp", "cin", S + E, U, self.act, ["c1", "c2", "c3"][:len(U)], colmap=self.cat_map,
                                   first_grad_ranges=[zc], tag="critic")
        last_a, last_c = ["a1", "a2", "a3"][len(U) - 1], ["c1", "c2", "c3"][len(U) - 1]
        g.buffer("value", 1)
        g.buffer("mu", self.actions_num)
        lins["value"] = g.linear(Linear(book, "a2c_network.value", U[-1], 1), last_c, "value", grad_ranges=[(0, U[-1], self.act, last_c, 0)], tag="critic")
        lins["mu"] = g.linear(Linear(book, "a2c_network.mu", U[-1], self.actions_num), last_a, "mu", grad_ranges=[(0, U[-1], self.act, last_a, 0)], tag="dec")
        # _build_z_mlp (:469-521): encoder, its heads, the learned prior and its heads
        lins["z_mlp"] = g.mlp("a2c_network.z_mlp", "x", self.obs_size, T, self.task_act, ["e1", "e2", "e3"][:len(T)],
                              final_linear=5 * E, final_dst="zenc", tag="enc")
        g.buffer("zheads", 2 * E)
        lins["zheads"] = g.linear(Linear(book, "a2c_network.z_heads", 5 * E, 2 * E), "zenc", "zheads", grad_ranges=[(0, 5 * E, ACT_NONE, None, 0)], tag="enc")
        if self.prior_mode != K.PRIOR_NONE:
            lins["z_prior"] = g.mlp("a2c_network.z_prior", "x", S, T, self.task_act, ["p1", "p2", "p3"][:len(T)], tag="prior")
            last_p = ["p1", "p2", "p3"][len(T) - 1]
            # learned: [z_prior_mu; z_prior_logvar] stacked; fixed: z_prior_mu alone, there is no z_prior_logvar (:529-533)
            pw, pname = (2 * E, "a2c_network.z_prior_heads") if self.prior_mode == K.PRIOR_LEARNED else (E, "a2c_network.z_prior_mu")
            g.buffer("pheads", pw)
            lins["pheads"] = g.linear(Linear(book, pname, T[-1], pw), last_p, "pheads", grad_ranges=[(0, T[-1], self.task_act, last_p, 0)], tag="prior")
        # _build_critic_z_mlp (:559-580): its final Linear writes the z slot of the critic's concat buffer
        lins["critic_z_mlp"] = g.mlp("a2c_network.critic_z_mlp", "x", self.obs_size, T, self.task_act, ["q1", "q2", "q3"][:len(T)],
                                     final_linear=E, final_dst="cin", final_dst_col=self.z_col, tag="critic_z")
        return {"graph": g, "lins": lins}

    def _plans(self, g):
        plans = {"fwd_enc": g.forward_plan({"enc"}), "fwd_dec": g.forward_plan({"dec"}),
                 "fwd_critic": _concat_plans(g.forward_plan({"critic_z"}), g.forward_plan({"critic"})),
                 "bwd_dec": g.backward_plan({"dec"}), "bwd_enc": g.backward_plan({"enc"}),
                 "bwd_critic": _concat_plans(g.backward_plan({"critic"}), g.backward_plan({"critic_z"}))}
        if self.prior_mode != K.PRIOR_NONE:                     # without a prior there is no sub-network, no plan, no gradient slab
            plans.update(fwd_prior=g.forward_plan({"prior"}), bwd_prior=g.backward_plan({"prior"}))
        return plans

    def _names(self):
        """The stacked heads under the reference's names: z_heads = [z_mu; z_logvar], z_prior_heads = [z_prior_mu; z_prior_logvar]."""
        E = self.embedding_size
        out = {}
        for n in self.book.params:
            stem, kind = n.rsplit(".", 1)
            if stem in ("a2c_network.z_heads", "a2c_network.z_prior_heads"):
                stem = stem[:-len("heads")]
                out[f"{stem}mu.{kind}"] = (n, slice(0, E))
                out[f"{stem}logvar.{kind}"] = (n, slice(E, 2 * E))
            else:
                out[n] = (n, None)
        return out

    # ------------------------------------------------------------------ head algebra (form_embedding :82-121, compute_prior :226-241)
    def split_heads(self, heads, prior=False):
        """(mu, logvar) of a heads buffer as the reference's form_embedding / compute_prior return them.  ``prior`` under a fixed prior: the
        (projected) mean and the constant, unclamped log-variance (:237-241)."""
        E = self.embedding_size
        if prior and self.prior_mode == K.PRIOR_FIXED:
            mu = heads[:, :E]
            if self.sphere_prior:
                mu = mu / (torch.norm(mu, dim=-1, keepdim=True) / self.embedding_norm + 1e-8)
            return mu, torch.ones_like(mu) * self.vae_prior_fixed_logvar
        mu, logvar = heads[:, :E], heads[:, E:2 * E]
        if self.use_vae_clamped_prior:
            logvar = torch.clamp(logvar, min=-5, max=self.vae_var_clamp_max)
        return mu, logvar

    def head_modes(self):
        """The mode keywords of the three vae_head launches (kernels.vae_embed takes the posterior pair only)."""
        return dict(prior_mode=self.prior_mode, prior_fixed_logvar=self.vae_prior_fixed_logvar, sphere_prior=self.sphere_prior,
                    embedding_norm=self.embedding_norm)
