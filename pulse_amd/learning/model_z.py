"""Adapter that gives the PULSE VAE network (network_z.AMPZNetwork) the model interface CommonAgent /
AMPAgent drive: workspace(m, train) / forward / eval_critic / backward over one flat parameter buffer.

Forward of the policy follows AMPZBuilder.Network.eval_actor (amp_network_z_builder.py:422-467):
encoder plan -> form_embedding (log-var clamp, re-parameterisation with fresh N(0,1) noise, :82-121) ->
cat(self_obs, z) -> decoder plan -> mu.  The (B,32) head algebra is two fused launches (pulse_amd/csrc/vae_head.hip):
pulse_vae_embed on the way forward, pulse_vae_head_backward (d z / d mu, d z / d logvar with the clamp mask, plus the KL / AR(1) /
regulariser terms of _optimize_kin) when the decoder's input gradient comes back from the GEMM plans.  No autograd tape.  The network's
prior mode (learned / fixed / none) and its two sphere switches travel to the launches as compile-time-folded modes (net.head_modes()).

Generation (form_embedding under flags.debug, :101-119): with ``z_source`` 'prior' / 'prior_mean' / 'normal' the latent comes from the prior
(pulse_vae_embed_prior) and the encoder plan is not launched: prior plan -> one head launch -> decoder plan.  Inference only.
"""
import torch

from .. import kernels as K

from .graph import GraphModel
from .network_z import AMPZNetwork, check_z_source


class AMPZModel(GraphModel):
    network = AMPZNetwork

    def __init__(self, params, *, generator=None, **kw):
        super().__init__(params, **kw)
        self.embedding_size = self.net.embedding_size
        self.generator = generator
        self._z_source, self._prior_logvar = "posterior", None

    # ---- where z comes from: the encoder's posterior (training, tracking) or the prior (generation; inference only)
    @property
    def z_source(self):
        return self._z_source

    @z_source.setter
    def z_source(self, value):
        self.set_z_source(value, self._prior_logvar)

    @property
    def prior_logvar(self):
        return self._prior_logvar

    @prior_logvar.setter
    def prior_logvar(self, value):
        self.set_z_source(self._z_source, value)

    def set_z_source(self, z_source, prior_logvar=None):
        """Both switches at once, validated against the network's prior (network_z.check_z_source) before either changes."""
        check_z_source(z_source, prior_logvar, self.net.prior_mode)
        self._z_source, self._prior_logvar = z_source, None if prior_logvar is None else float(prior_logvar)

    def _fill_workspace(self, ws, m):
        super()._fill_workspace(ws, m)
        ws["z_noise"] = None                                        # (a test's injected re-parameterisation noise, _embed)
        zc = self.net.z_col
        ws["z"] = ws["g"].act_bufs["ain"][:, zc:zc + self.net.embedding_size]     # the z the decoder read, whatever its source
        ws["z_record"] = None                                       # (a recorder's (m, E) rows: the prior launch writes z there as well)

    def _noise(self, ws, m):
        """ws['z_noise'] when a test injected it, a fresh draw from self.generator otherwise."""
        if ws["z_noise"] is not None:
            return ws["z_noise"]
        eps = ws.get("_eps_buf")
        if eps is None:
            eps = ws["_eps_buf"] = torch.empty(m, self.net.embedding_size, device=self.device)
        eps.normal_(generator=self.generator)
        return eps

    def _embed_prior(self, ws):
        """form_embedding under flags.debug (amp_network_z_builder.py:101-119): the prior plan (when there is a prior), then one launch that
        draws z from it and places z and the self observation in the decoder's (and the critic's) concat buffer.  No encoder plan."""
        net, g = self.net, ws["g"]
        m = ws["x"].shape[0]
        pheads = None
        if net.prior_mode != K.PRIOR_NONE:
            ws["G"]["fwd_prior"].run()
            pheads = g.act_bufs["pheads"]
        eps = None if self._z_source == "prior_mean" else self._noise(ws, m)
        K.vae_embed_prior(pheads, ws["x"], g.act_bufs["ain"], rows=m, embedding_size=net.embedding_size, self_obs_size=net.self_obs_size,
                          z_col=net.z_col, eps=eps, cin=g.act_bufs["cin"], z_out=ws["z_record"], clamp=net.use_vae_clamped_prior,
                          clamp_max=net.vae_var_clamp_max, logvar_override=self._prior_logvar, sphere_posterior=net.use_vae_sphere_posterior,
                          **net.head_modes())
        ws["eps"] = eps

    def _embed(self, ws):
        """form_embedding (amp_network_z_builder.py:79-121) on the encoder heads in one launch: clamp, re-parameterise, and place z and the
        self observation in the decoder's (and the critic's) concat buffer.  The noise is ws['z_noise'] when a test injected it, a fresh
        draw otherwise; z = mu in test mode."""
        net, g = self.net, ws["g"]
        E, S = net.embedding_size, net.self_obs_size
        heads = g.act_bufs["zheads"]
        m = heads.shape[0]
        eps = None if getattr(self, "deterministic_z", False) else self._noise(ws, m)
        K.vae_embed_modes(heads, ws["x"], g.act_bufs["ain"], rows=m, embedding_size=E, self_obs_size=S, z_col=net.z_col, eps=eps, cin=g.act_bufs["cin"],
                          clamp=net.use_vae_clamped_prior, clamp_max=net.vae_var_clamp_max, sphere_posterior=net.use_vae_sphere_posterior,
                          embedding_norm=net.embedding_norm)
        ws["eps"] = eps

    def forward_actor(self, ws, m, need_grad=None):
        if self._z_source == "posterior":
            ws["G"]["fwd_enc"].run()
            self._embed(ws)
        else:                                                        # generation: the encoder plan is not launched
            self._embed_prior(ws)
        ws["G"]["fwd_dec"].run()

    def eval_critic(self, ws, m):
        g, S = ws["g"], self.net.self_obs_size
        g.act_bufs["cin"][:, :S].copy_(ws["x"][:, :S])
        ws["G"]["fwd_critic"].run()

    def forward(self, ws, m):
        self.forward_actor(ws, m)                                    # (_embed also fills the critic's self-observation columns)
        ws["G"]["fwd_critic"].run()

    def compute_prior(self, ws, need_grad=False):
        """compute_prior (:226-241): runs the prior MLP; the raw heads ([mu | logvar] learned, mu fixed) stay in the graph buffer 'pheads'
        (split_heads clamps / projects).  Without a prior there is nothing to run: None."""
        if self.net.prior_mode == K.PRIOR_NONE:
            return None
        ws["G"]["fwd_prior"].run()
        return self.net.split_heads(ws["g"].act_bufs["pheads"], prior=True)

    # ---- backward
    def backward_actor(self, ws, kin=None):
        """d loss/d mu is already in ws['dmu'].  Back-propagates decoder -> z -> encoder.  ``kin``: the head-level terms of _optimize_kin
        (dict c_kl, c_ar1, c_regu, progress, horizon) whose gradients join the re-parameterisation path at the encoder / prior heads; one
        launch of pulse_vae_head_backward either way."""
        if self._z_source != "posterior":
            raise RuntimeError(f"backward_actor with z_source {self._z_source!r}: a latent drawn from the prior is inference only (there is no "
                               "re-parameterisation path through the encoder to differentiate); set z_source = 'posterior' to train")
        g, net = ws["g"], self.net
        E, zc = net.embedding_size, net.z_col
        ws["G"]["bwd_dec"].run()
        dz = g.grad("ain")[:, zc:zc + E]
        heads = g.act_bufs["zheads"]
        kw = dict(rows=heads.shape[0], embedding_size=E, eps=ws["eps"], dz=dz, clamp=net.use_vae_clamped_prior, clamp_max=net.vae_var_clamp_max,
                  sphere_posterior=net.use_vae_sphere_posterior, **net.head_modes())
        if kin is not None:
            if net.prior_mode != K.PRIOR_NONE:
                kw.update(pheads=g.act_bufs["pheads"], dpheads=g.grad("pheads"))
            kw.update(progress=kin.get("progress"), horizon=kin.get("horizon", 1),
                      c_kl=kin["c_kl"], c_ar1=kin.get("c_ar1", 0.0), c_regu=kin.get("c_regu", 0.0))
        K.vae_head_backward_modes(heads, g.grad("zheads"), **kw)
        ws["G"]["bwd_enc"].run()

    def backward_prior(self, ws):
        if self.net.prior_mode != K.PRIOR_NONE:
            ws["G"]["bwd_prior"].run()                                  # d loss / d prior heads was written by backward_actor(kin=...)

    def backward(self, ws, m, grad_scale=1.0, sq_partials=None, on_bucket=None):
        """PPO backward: actor (through the VAE) + critic; weight gradients of untouched sub-nets (the prior: kin pass only) are zero.
        ``sq_partials``: the gradient reduce also leaves the norm clip's per-block sums of squares there; returns True when it did."""
        self.backward_actor(ws)
        ws["G"]["bwd_critic"].run()
        return self._reduce(grad_scale, self._untouched(ws, ("dec", "enc", "critic", "critic_z")), sq_partials)
