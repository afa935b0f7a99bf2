"""GPU: generation from the PULSE prior -- pulse_vae_embed_prior (pulse_amd/csrc/vae_head.hip), AMPZModel.z_source and the player's generate().

The yardstick is never the kernel: tests/golden/prior_sampling.npz (outputs of the reference's own form_embedding under flags.debug,
amp_network_z_builder.py:101-119) where the reference has a statement that runs, and tests/prior_sampling_model.py (held to that fixture bit
for bit by tests/test_prior_sampling_cpu.py) elsewhere.  The prior-mean and constant-log-variance variants are commented out in the reference
(:109-111): for them the restatement IS the yardstick.

Tolerance: z within 2e-6 of its maximum, the figure tests/test_vae_head_gpu.py holds the posterior kernel to (one exp, one multiply, one
add; the projection adds a 32-term sum, a square root and a divide).  The copied self-observation columns, the z_out copy and everything the
launch must not touch are compared exactly; the outputs are pre-filled with NaN.

The model's mean: the kernel's exp is not torch's, so the latent of a sampled source matches the restatement to that tolerance, not to the
bit; 'mu is the decoder plan on that z' is therefore shown bit for bit with the restated z written by hand where the restatement needs no
exp and no row norm (z = the prior's mean head; z = the noise), and with the recorded ws['z'] -- itself held to the restatement -- written by
hand everywhere."""
import itertools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden_prior_sampling as GP  # noqa: E402
import prior_sampling_model as PM  # noqa: E402
import vae_variants_model as VM  # noqa: E402
from pulse_amd import _lib, configs  # noqa: E402
from pulse_amd import kernels as K  # noqa: E402
from pulse_amd.learning.model_z import AMPZModel  # noqa: E402

pytestmark = pytest.mark.gpu

NORM, FIXED_LV, CLAMP_MAX = 1.7, -0.6, 2.0
PRIORS = {"learned": (K.PRIOR_LEARNED, False), "fixed": (K.PRIOR_FIXED, False), "fixed_sphere": (K.PRIOR_FIXED, True), "none": (K.PRIOR_NONE, False)}
CASES = [(p, s) for p in PRIORS for s in (False, True)]
IDS = [f"{p}-{'sphere' if s else 'gauss'}" for p, s in CASES]
NAN = float("nan")


def _pitched(t, extra, dev):
    """``t`` on the device as a view of a NaN-filled allocation whose row pitch exceeds the width by ``extra``."""
    if t is None:
        return None
    buf = torch.full((t.shape[0], t.shape[1] + extra), NAN, device=dev)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf[:, :t.shape[1]]


def _launch_and_check(dev, *, prior, post, mu, lv, eps, x, S, zc, want, extra=0, with_cin=True, with_zout=True, clamp=True, override=None, what=""):
    """One launch on NaN-filled outputs: the exact claims, then z against ``want`` (CPU) within 2e-6 of its maximum."""
    mode, sprior = PRIORS[prior]
    rows, E = want.shape
    ph = None if mode == K.PRIOR_NONE else _pitched(torch.cat([mu, lv], dim=1) if mode == K.PRIOR_LEARNED else mu, extra, dev)
    e, xd = _pitched(eps, extra, dev), _pitched(x, extra, dev)
    ain = torch.full((rows, zc + E + 3 + extra), NAN, device=dev)
    cin = torch.full((rows, zc + E + 3 + extra), NAN, device=dev) if with_cin else None
    zo = torch.full((rows, E + extra), NAN, device=dev) if with_zout else None
    K.vae_embed_prior(ph, xd, ain, rows=rows, embedding_size=E, self_obs_size=S, z_col=zc, eps=e, cin=cin, z_out=None if zo is None else zo[:, :E],
                      prior_mode=mode, prior_fixed_logvar=FIXED_LV, clamp=clamp, clamp_max=CLAMP_MAX, logvar_override=override, sphere_prior=sprior,
                      sphere_posterior=post, embedding_norm=NORM)
    assert torch.equal(ain[:, :S], xd[:, :S]), what
    assert torch.isnan(ain[:, S:zc]).all() and torch.isnan(ain[:, zc + E:]).all(), what
    if with_cin:
        assert torch.equal(cin[:, :S], xd[:, :S]) and torch.isnan(cin[:, S:]).all(), what
    z = ain[:, zc:zc + E]
    if with_zout:
        assert torch.equal(zo[:, :E], z) and torch.isnan(zo[:, E:]).all(), what
    err, scale = (z.cpu() - want).abs().max().item(), want.abs().max().item()
    print(f"{what}: z error {err:.3e}, bound {2e-6 * scale:.3e}")
    assert err <= 2e-6 * scale, (what, err, scale)
    return z


def _heads(rows, E, seed):
    """Raw prior heads, noise and observation rows; the log-variances on both sides of [-5, 2] and not within 1e-3 of its edges."""
    g = torch.Generator().manual_seed(seed)
    mu, lv = torch.randn(rows, E, generator=g), torch.randn(rows, E, generator=g) * 3.0
    for edge in (-5.0, CLAMP_MAX):
        lv[(lv - edge).abs() < 1e-3] = edge + 0.01
    if rows * E >= 7:
        lv.view(-1)[0], lv.view(-1)[1], lv.view(-1)[2] = -7.5, 3.25, 0.5
    eps = torch.randn(rows, E, generator=g)
    x = torch.randn(rows, 365, generator=g)
    return mu, lv, eps, x


def _want(prior, post, mu, lv, eps, **kw):
    return PM.z_from_prior_heads(mu, lv, eps, prior="fixed" if prior == "fixed_sphere" else prior, clamp_max=CLAMP_MAX, fixed_logvar=FIXED_LV,
                                 sphere_prior=PRIORS[prior][1], sphere_posterior=post, embedding_norm=NORM, **kw)


# --------------------------------------------------------------------------------------------------------------------------- the kernel
@pytest.fixture(scope="module")
def fx():
    return {k: torch.from_numpy(v) for k, v in GP.load().items() if v.ndim == 2}


@pytest.mark.parametrize("prior,post", CASES, ids=IDS)
def test_kernel_against_the_reference_fixture(dev, fx, prior, post):
    assert (GP.GV.NORM, GP.GV.FIXED_LOGVAR) == (NORM, FIXED_LV)
    obs = GP.inputs()["obs"]
    S = GP.GV.SIZES["self_obs_size"]
    mu = fx.get(f"heads/{prior}/mu")
    lv = fx.get("heads/learned/logvar") if prior == "learned" else None
    _launch_and_check(dev, prior=prior, post=post, mu=mu, lv=lv, eps=fx["eps"], x=obs, S=S, zc=12, want=fx[f"z/{prior}/{'sphere' if post else 'gauss'}"],
                      what=f"fixture {prior} post={post}")


@pytest.mark.parametrize("prior,post", CASES, ids=IDS)
def test_kernel_row_and_lane_edges(dev, prior, post):
    """rows around the eight of a workgroup, latents that fill / half fill / barely use the 32 lanes, with and without pad columns before z,
    pitched and dense buffers, with and without the optional outputs."""
    shapes = list(itertools.product((1, 7, 8, 9, 17), (32, 20, 1), (358, 360)))
    seen = set()
    for i, (rows, E, S) in enumerate(shapes):
        extra, with_cin, with_zout = (5 if i % 2 == 0 else 0), (i // 2) % 2 == 0, (i // 4) % 2 == 0
        seen.add((extra > 0, with_cin, with_zout))
        mu, lv, eps, x = _heads(rows, E, seed=100 + i)
        _launch_and_check(dev, prior=prior, post=post, mu=mu, lv=lv, eps=eps, x=x, S=S, zc=360, want=_want(prior, post, mu, lv, eps), extra=extra,
                          with_cin=with_cin, with_zout=with_zout, what=f"{prior} post={post} rows={rows} E={E} S={S} pitch+{extra}")
    assert len(seen) == 8                                        # every combination of pitched / cin / z_out was launched


@pytest.mark.parametrize("prior,post", [c for c in CASES if c[0] != "none"], ids=[i for i in IDS if not i.startswith("none")])
def test_kernel_prior_mean_temperature_and_unclamped(dev, prior, post):
    """The variants the reference keeps commented out (:109-111) and the clamp switch: the restatement is the yardstick."""
    for rows, E in ((17, 32), (9, 20)):
        mu, lv, eps, x = _heads(rows, E, seed=7 + rows)
        kw = dict(dev=dev, prior=prior, post=post, mu=mu, lv=lv, x=x, S=358, zc=360)
        z_mean = _launch_and_check(eps=None, want=_want(prior, post, mu, lv, None), what=f"prior mean {prior} post={post} E={E}", **kw)
        if not post and prior != "fixed_sphere":
            assert torch.equal(z_mean.cpu(), mu)                   # nothing is computed: the mean head itself
        z_full = _launch_and_check(eps=eps, want=_want(prior, post, mu, lv, eps), what=f"sampled {prior} post={post} E={E}", **kw)
        for c in (-2.3, -1.5):
            z_c = _launch_and_check(eps=eps, override=c, want=_want(prior, post, mu, lv, eps, logvar_override=c),
                                    what=f"logvar {c} {prior} post={post} E={E}", **kw)
            assert not torch.equal(z_c, z_full)
        if prior == "learned":
            assert (lv < -5).any() and (lv > CLAMP_MAX).any()
            z_raw = _launch_and_check(eps=eps, clamp=False, want=_want(prior, post, mu, lv, eps, clamp=False), what=f"clamp off post={post} E={E}", **kw)
            assert not torch.equal(z_raw, z_full)


def test_kernel_argument_errors_launch_nothing(dev):
    rows, E, S, zc = 16, 32, 37, 40
    mu, lv, eps, x = _heads(rows, 33, seed=1)
    ph, e33, xd = torch.cat([mu, lv], dim=1).to(dev), eps.to(dev), x.to(dev)
    ain, cin, zo = (torch.full((rows, 80), NAN, device=dev) for _ in range(3))
    base = dict(rows=rows, embedding_size=E, self_obs_size=S, z_col=zc, cin=cin, z_out=zo)
    bad = [("eps must be given", dict(base, pheads=None, eps=None, prior_mode=K.PRIOR_NONE)),                       # PRIOR_NONE without noise
           ("embedding_size <= 32", dict(base, pheads=ph, eps=e33, embedding_size=33)),
           ("needs the prior heads", dict(base, pheads=None, eps=e33, prior_mode=K.PRIOR_LEARNED)),
           ("pheads_stride too small", dict(base, pheads=ph[:, :40].contiguous(), eps=e33, prior_mode=K.PRIOR_LEARNED)),   # 40 < 2E
           ("prior_mode", dict(base, pheads=ph, eps=e33, prior_mode=3)),
           ("embedding_norm", dict(base, pheads=ph, eps=e33, sphere_posterior=True, embedding_norm=0.0))]
    for msg, kw in bad:
        pheads = kw.pop("pheads")
        with pytest.raises(_lib.PulseLibraryError, match=f"status -1.*{msg}"):                                      # PULSE_ERR_INVALID_ARG
            K.vae_embed_prior(pheads, xd, ain, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(ain).all() and torch.isnan(cin).all() and torch.isnan(zo).all()
    K.vae_embed_prior(ph, xd, ain, rows=0, embedding_size=E, self_obs_size=S, z_col=zc)                              # zero rows: a no-op
    assert torch.isnan(ain).all()


# --------------------------------------------------------------------------------------------------------------------------- the model
def _restatement(variant):
    v = configs.VAE_VARIANTS[variant]
    return VM.VariantNetZ(use_vae_prior=v.get("use_vae_prior", True), use_vae_fixed_prior=v.get("use_vae_fixed_prior", False),
                          use_vae_sphere_prior=v.get("use_vae_sphere_prior", False), use_vae_sphere_posterior=v.get("use_vae_sphere_posterior", False),
                          vae_prior_fixed_logvar=v.get("vae_prior_fixed_logvar", 0), embedding_norm=v.get("embedding_norm", 1))


def _model(dev, variant, seed=5):
    torch.manual_seed(seed)
    ref = _restatement(variant)
    detail = dict({k: configs.ENV_IM_VAE[k] for k in ("embedding_size", "embedding_norm", "z_type", "use_vae_prior", "use_vae_clamped_prior",
                                                       "vae_var_clamp_max")}, **configs.vae_variant_env(variant))
    gen = torch.Generator(device=dev).manual_seed(seed)
    model = AMPZModel(configs.NETWORK_Z, actions_num=69, self_obs_size=358, task_obs_size=576, task_obs_size_detail=detail, device=dev, generator=gen)
    model.load_state_dict(ref.state_dict_ref())
    return model.eval(), ref


def _feed(model, n, seed=9):
    g = torch.Generator().manual_seed(seed)
    obs, noise = torch.randn(n, 934, generator=g).clamp(-5, 5), torch.randn(n, 32, generator=g)
    ws = model.workspace(n, train=False)
    ws["x"].zero_()
    ws["x"][:, :934] = obs.to(model.device)
    ws["z_noise"] = noise.to(model.device)
    return ws, obs, noise


def _poison(bufs, net, names):
    """NaN into the named activation buffers; of the two concat buffers only the self-observation and latent columns (the pad columns
    between them meet zero weights in the first layer's GEMM and have to stay finite)."""
    S, zc, E = net.self_obs_size, net.z_col, net.embedding_size
    for k in names:
        if k in ("ain", "cin"):
            bufs[k][:, :S] = NAN
            bufs[k][:, zc:zc + E] = NAN
        else:
            bufs[k].fill_(NAN)


MODEL_CASES = [("learned", "prior"), ("learned", "prior_mean"), ("sphere_post", "prior"), ("fixed", "prior"), ("fixed", "prior_mean"),
               ("fixed_sphere_post", "prior"), ("none", "normal"), ("none_sphere_post", "normal")]


@pytest.mark.parametrize("variant,source", MODEL_CASES, ids=[f"{v}-{s}" for v, s in MODEL_CASES])
def test_model_generates_without_the_encoder(dev, variant, source):
    n, E = 24, 32
    model, ref = _model(dev, variant)
    net = model.net
    zc, S = net.z_col, net.self_obs_size
    ws, obs, noise = _feed(model, n)
    bufs = ws["g"].act_bufs
    model.z_source = source
    _poison(bufs, net, ("zheads", "mu", "ain"))
    model.forward_actor(ws, n)
    assert torch.isnan(bufs["zheads"]).all()                           # the encoder plan never ran
    mu = ws["mu"].clone()
    assert torch.isfinite(mu).all() and torch.equal(bufs["ain"][:, :S], ws["x"][:, :S])
    z = ws["z"].clone()
    assert z.data_ptr() != ws["z"].data_ptr() and torch.equal(z, bufs["ain"][:, zc:zc + E])
    # ---- z against the restatement on the launch's own inputs: the prior plan's heads buffer and the injected noise
    eps = None if source == "prior_mean" else noise
    if net.prior_mode == K.PRIOR_NONE:
        want = PM.z_from_prior_heads(None, None, eps, **PM.net_modes(ref))
    else:
        ph = bufs["pheads"].cpu()
        want = PM.z_from_prior_heads(ph[:, :E], ph[:, E:2 * E] if net.prior_mode == K.PRIOR_LEARNED else None, eps, **PM.net_modes(ref))
    err, scale = (z.cpu() - want).abs().max().item(), want.abs().max().item()
    print(f"{variant} {source}: z error {err:.3e}, bound {2e-6 * scale:.3e}")
    assert err <= 2e-6 * scale
    exact = not net.use_vae_sphere_posterior and not net.sphere_prior and source in ("prior_mean", "normal")
    if exact:
        assert torch.equal(z.cpu(), want)
    # ---- mu is the decoder plan on cat(self_obs, z), z written by hand
    for by_hand in ([want.to(dev)] if exact else []) + [z]:
        _poison(bufs, net, ("ain", "mu"))
        bufs["ain"][:, :S] = ws["x"][:, :S]
        bufs["ain"][:, zc:zc + E] = by_hand
        ws["G"]["fwd_dec"].run()
        assert torch.equal(ws["mu"], mu)
    # ---- and end to end it is the restated network's mean (the bound of the same-depth prior -> z -> decoder path in
    # tests/test_vae_variants_gpu.py::test_compute_z_actions_matches_the_restatement)
    with torch.no_grad():
        mu_ref, z_ref = PM.generate_mu(ref, obs, eps)
    e_mu, s_mu = (mu.cpu() - mu_ref).abs().max().item(), mu_ref.abs().max().item()
    print(f"{variant} {source}: mu error {e_mu:.3e} of {s_mu:.3e}; z vs the CPU network {(z.cpu() - z_ref).abs().max().item():.3e}")
    assert e_mu <= 5e-5 * (s_mu + 1e-12)
    # ---- the full forward fills the critic's self observation too; inference only
    model.forward(ws, n)
    assert torch.equal(bufs["cin"][:, :S], ws["x"][:, :S]) and torch.isfinite(ws["val"]).all() and torch.isnan(bufs["zheads"]).all()
    ws["dmu"].zero_()
    with pytest.raises(RuntimeError, match="inference only"):
        model.backward_actor(ws)


def test_model_temperature_and_fresh_noise(dev):
    n, E = 24, 32
    model, ref = _model(dev, "learned")
    ws, obs, noise = _feed(model, n)
    model.set_z_source("prior", prior_logvar=-2.3)
    model.forward_actor(ws, n)
    ph = ws["g"].act_bufs["pheads"].cpu()
    want = PM.z_from_prior_heads(ph[:, :E], ph[:, E:], noise, logvar_override=-2.3, **PM.net_modes(ref))
    assert (ws["z"].cpu() - want).abs().max().item() <= 2e-6 * want.abs().max().item()
    assert torch.equal(ws["eps"], ws["z_noise"])
    # no injected noise: a fresh draw from the model's generator per call, reproducible from its seed
    ws["z_noise"] = None
    model.set_z_source("prior")
    model.generator.manual_seed(77)
    model.forward_actor(ws, n)
    z1, e1 = ws["z"].clone(), ws["eps"].clone()
    model.forward_actor(ws, n)
    z2 = ws["z"].clone()
    model.generator.manual_seed(77)
    model.forward_actor(ws, n)
    assert not torch.equal(z1, z2) and torch.equal(ws["z"], z1) and torch.equal(ws["eps"], e1)
    assert 0.5 < e1.std().item() < 1.5 and abs(e1.mean().item()) < 0.3
    # the options are checked against the network when they are set
    with pytest.raises(ValueError, match="without a prior"):
        model.z_source = "normal"
    with pytest.raises(ValueError, match="prior_logvar"):
        model.set_z_source("prior_mean", prior_logvar=-1.5)
    assert model.z_source == "prior" and model.prior_logvar is None
    none_model, _ = _model(dev, "none")
    with pytest.raises(ValueError, match=r"use_vae_prior.*use_vae_fixed_prior"):
        none_model.z_source = "prior"


@pytest.mark.parametrize("variant", ["learned", "fixed_sphere_post"])
def test_posterior_source_is_the_model_as_it_was(dev, variant):
    """z_source 'posterior' -- set explicitly, or come back to after generating -- gives the bits of a model that was never told about it."""
    n = 24
    outs = []
    for touch in (None, "set", "round_trip"):
        model, _ = _model(dev, variant)
        ws, _, _ = _feed(model, n)
        if touch == "set":
            model.z_source = "posterior"
        elif touch == "round_trip":
            model.z_source = "prior"
            model.forward(ws, n)
            model.z_source = "posterior"
        assert model.z_source == "posterior" and model.prior_logvar is None
        _poison(ws["g"].act_bufs, model.net, ("zheads", "mu", "ain", "cin"))
        model.train()
        model.forward(ws, n)
        ws["dmu"].copy_(torch.linspace(-1e-3, 1e-3, n * 69, device=dev).view(n, 69))
        model.backward_actor(ws)                                     # and it trains as before
        outs.append([ws["g"].act_bufs[k].clone() for k in ("zheads", "mu", "ain", "cin")] + [ws["val"].clone(), ws["g"].grad("zheads").clone()])
        assert torch.isfinite(outs[-1][0]).all() and torch.equal(ws["z"], ws["g"].act_bufs["ain"][:, model.net.z_col:model.net.z_col + 32])
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


# --------------------------------------------------------------------------------------------------------------------------- the player
def _generate(dev, seed, steps=8, **kw):
    torch.manual_seed(1)              # the network's initial weights stand in for a checkpoint: the same ones whatever the player's seed
    player = configs.make_player("cfg3_small", device=str(dev), seed=seed, num_envs_override=16, **kw)
    return player, player.generate(steps, record=True)


def test_player_generates_motion_from_the_prior(dev):
    player, out = _generate(dev, 11, z_source="prior")
    assert player.z_source == "prior" and player.model.z_source == "prior"
    J = player.env.task.sim.rigid_body_state.shape[1]
    assert out["steps"] == 8 and isinstance(out["resets"], int) and 0 <= out["resets"] <= 8 * 16
    z, rb = out["z"], out["rb"]
    assert z.shape == (8, 16, 32) and rb.shape == (8, 16, J, 13) and z.is_cuda and rb.is_cuda
    assert torch.isfinite(z).all() and torch.isfinite(rb).all()
    assert (z[:, 1:] != z[:, :1]).any(dim=-1).all() and (z[1:] != z[:1]).any(dim=-1).all()        # between envs, between steps
    assert not torch.equal(rb[0], rb[-1])
    assert torch.equal(z[-1], player.model.workspace(16, train=False)["z"])                        # the record is the z that was used
    assert set(player.generate(2)) == {"steps", "resets"}
    _, again = _generate(dev, 11, z_source="prior")
    _, other = _generate(dev, 12, z_source="prior")
    assert torch.equal(again["z"], z) and torch.equal(again["rb"], rb) and again["resets"] == out["resets"]
    assert not torch.equal(other["z"], z)


def test_player_prior_mean_is_compute_priors_mean(dev):
    player, out = _generate(dev, 11, steps=4, z_source="prior_mean")
    ws = player.model.workspace(16, train=False)                      # still holds the last step's normalised observation
    mean, _ = player.model.compute_prior(ws)
    assert torch.equal(out["z"][-1], mean) and (out["z"][1:] != out["z"][:1]).any(dim=-1).all()
    # the default source goes through the encoder and records its z as well
    player, out = _generate(dev, 11, steps=2)
    assert player.z_source == "posterior" and out["z"].shape == (2, 16, 32) and torch.isfinite(out["z"]).all()


@pytest.mark.parametrize("variant,source,radius", [("fixed", "prior", None), ("fixed_sphere_post", "prior", 2.0), ("none", "normal", None),
                                                   ("none_sphere_post", "normal", 2.0)])
def test_player_runs_the_other_priors(dev, variant, source, radius):
    player, out = _generate(dev, 3, steps=4, z_source=source, env_overrides=configs.vae_variant_env(variant))
    assert out["z"].shape == (4, 16, 32) and torch.isfinite(out["z"]).all() and torch.isfinite(out["rb"]).all()
    assert (out["z"][:, 1:] != out["z"][:, :1]).any(dim=-1).all()
    if radius is not None:
        assert (out["z"].norm(dim=-1) - radius).abs().max().item() <= 1e-5
    if variant.startswith("none"):
        assert "fwd_prior" not in player.model.workspace(16, train=False)["G"]
    run = player.run(3)                                                # the evaluation loop is what it was
    assert set(run) == {"games", "av_reward"}


def test_generate_on_a_network_without_a_latent_records_the_bodies_only(dev):
    player = configs.make_player("cfg1", device=str(dev), seed=3)
    out = player.generate(3, record=True)
    assert set(out) == {"steps", "resets", "rb"} and out["rb"].shape[:2] == (3, 64) and torch.isfinite(out["rb"]).all()
