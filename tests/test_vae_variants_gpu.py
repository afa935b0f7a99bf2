"""GPU: the prior / posterior variants of the PULSE VAE head kernels (pulse_amd/csrc/vae_head.hip), of AMPAgent._optimize_kin and of
HumanoidZ.compute_z_actions.  The yardstick is the reference's formulas under torch autograd (tests/vae_variants_model.py, pinned to the
reference's method bodies by tests/test_vae_variants_cpu.py), never the kernel.

Kernel tolerances are those of tests/test_vae_head_gpu.py: losses 2e-5 relative, z 2e-6 of its maximum, head gradients 3e-6 * max + 1e-10.
The projected paths divide by a row norm, so their rounding error is set by the inputs: there the bound is the larger of that figure and
4x the error of the SAME formulas evaluated by fp32 autograd against fp64 on the same inputs (computed and printed by the test)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import vae_variants_model as VM  # noqa: E402
from oracle import agent_oracle as AO  # noqa: E402
from pulse_amd import configs  # noqa: E402
from pulse_amd import kernels as K  # noqa: E402

pytestmark = pytest.mark.gpu

NORM, FIXED_LV, CLAMP_MAX = 1.7, -0.6, 2.0
PRIORS = {"learned": (K.PRIOR_LEARNED, False), "fixed": (K.PRIOR_FIXED, False), "fixed_sphere": (K.PRIOR_FIXED, True), "none": (K.PRIOR_NONE, False)}
ZERO_ROW = 5                      # the row built to have z = 0 exactly (rows >= 7)


def _inputs(dev, rows, t, E, A=69, seed=0):
    g = torch.Generator().manual_seed(seed)
    zh = torch.randn(rows, 2 * E, generator=g)
    zh[:, E:] *= 3.0                                                        # raw log-variances on both sides of the clamp range [-5, 2]
    ph = torch.randn(rows, 2 * E, generator=g)
    ph[:, E:] *= 3.0
    for h in (zh, ph):                                                      # ... and not within 1e-3 of its edges
        lv = h[:, E:]
        for edge in (-5.0, CLAMP_MAX):
            lv[(lv - edge).abs() < 1e-3] = edge + 0.01
    pred, gt = torch.randn(rows, A, generator=g), torch.randn(rows, A, generator=g) * 0.4
    eps = torch.randn(rows, E, generator=g)
    dz = torch.randn(rows, E, generator=g) * 1e-3
    if rows > ZERO_ROW:
        zh[ZERO_ROW, :E] = 0.0
        eps[ZERO_ROW] = 0.0
    seqs = rows // t
    prog = torch.randint(0, 50, (seqs, 1), generator=g) + torch.arange(t)[None, :]
    if seqs > 4:
        prog[2, 5:] = torch.arange(t - 5)                                    # an episode seam inside sequence 2
        prog[4, :] = torch.arange(t)                                         # a sequence that starts at frame 0 (first frames are masked)
    d = dict(zh=zh, ph=ph, pred=pred, gt=gt, eps=eps, dz=dz, prog=prog.reshape(-1))
    for h in (zh, ph):
        lv = h[:, E:]
        assert (lv < -5).any() or rows < 7
        assert (((lv + 5).abs() >= 1e-3) & ((lv - CLAMP_MAX).abs() >= 1e-3)).all()
    if rows >= 7:
        assert (zh[:, E:] > CLAMP_MAX).any() and (zh[:, E:] < -5).any() and ((zh[:, E:] > -5) & (zh[:, E:] < CLAMP_MAX)).any()
    z = zh[:, :E] + torch.exp(0.5 * zh[:, E:].clamp(-5, CLAMP_MAX)) * eps
    nz = z.norm(dim=-1)
    keep = torch.ones(rows, dtype=torch.bool)
    if rows > ZERO_ROW:
        keep[ZERO_ROW] = False
        assert nz[ZERO_ROW] == 0
    assert (nz[keep] >= 0.5).all(), nz.min()
    assert (zh[:, :E].norm(dim=-1)[keep] >= 0.5).all() and (ph[:, :E].norm(dim=-1) >= 0.5).all()
    return {k: v.to(dev) for k, v in d.items()}, keep.to(dev)


def _formulas(d, *, prior, post, t, E, use_ar1, use_regu, dtype, test_mode=False, kld_w=0.01, ar1_w=0.005):
    """The reference's formulas under autograd in ``dtype``: loss terms, z, and the gradients of loss + <z', dz> w.r.t. the heads / pred."""
    mode, sprior = PRIORS[prior]
    c = lambda x: x.detach().to(dtype)
    zh, pred = c(d["zh"]).requires_grad_(True), c(d["pred"]).requires_grad_(True)
    pw = 2 * E if mode == K.PRIOR_LEARNED else E
    ph = c(d["ph"][:, :pw]).requires_grad_(True)
    gt, eps, dz, prog = c(d["gt"]), c(d["eps"]), c(d["dz"]), d["prog"]
    mb = zh.shape[0]
    qm, qv = zh[:, :E], torch.clamp(zh[:, E:], min=-5, max=CLAMP_MAX)
    z = qm + torch.exp(0.5 * qv) * eps
    if test_mode:
        z = qm
    if post:
        z = VM.project_to_norm(z, NORM)
    act = torch.norm(pred - gt, dim=-1).mean()
    pm = pv = None
    if mode == K.PRIOR_LEARNED:
        pm, pv = ph[:, :E], torch.clamp(ph[:, E:], min=-5, max=CLAMP_MAX)
    elif mode == K.PRIOR_FIXED:
        pm = VM.project_to_norm(ph, NORM) if sprior else ph
        pv = torch.ones_like(pm) * FIXED_LV
    if pm is not None:
        kld = AO.kl_multi(qm, qv, pm, pv).mean()
    else:
        kld = -0.5 * torch.sum(1 + qv - qm.pow(2) - qv.exp()) / mb
    ar1 = torch.zeros((), device=zh.device, dtype=dtype)
    if use_ar1:
        zs = qm.view(mb // t, t, -1)
        err = (zs[:, 1:] - zs[:, :-1] * 0.99).reshape(-1, E)
        idx = prog.view(mb // t, t, -1)
        bad = ((idx[:, 1:] - idx[:, :-1]) != 1).view(-1) | ((idx <= 2)[:, 1:] | (idx <= 2)[:, :-1]).view(-1)
        err = err * (~bad).to(dtype)[:, None]
        ar1 = torch.norm(err, dim=-1).mean()
    regu = torch.zeros((), device=zh.device, dtype=dtype)
    if use_regu:
        regu = ((pm ** 2).mean() + (qm ** 2).mean()) * 0.001 + ((pv ** 2).mean() + (qv ** 2).mean()) * 0.001
    loss = act + kld * kld_w + ar1 * ar1_w + regu * 0.005
    torch.autograd.backward([loss, z], [None, dz])
    return dict(act=act.detach(), kld=kld.detach(), ar1=ar1.detach(), regu=regu.detach(), z=z.detach(), dzh=zh.grad, dpred=pred.grad,
                dph=ph.grad if mode != K.PRIOR_NONE else None)


def _bound(got, want32, want64, keep, base, what, projected):
    """|got - want32| over the rows ``keep`` within base * max + 1e-10, or (projected paths) 4x the fp32-vs-fp64 error of the formulas."""
    g, w, w64 = got[keep].double(), want32[keep].double(), want64[keep]
    scale = w.abs().max().item()
    tol = base * scale + 1e-10
    if projected:
        margin = 4.0 * (w - w64).abs().max().item()
        print(f"{what}: base bound {tol:.3e}, 4 x fp32-vs-fp64 formula error {margin:.3e}, kernel error {(g - w).abs().max().item():.3e}")
        tol = max(tol, margin)
    err = (g - w).abs().max().item()
    assert err <= tol, (what, err, tol, scale)


CASES = [(p, s) for p in PRIORS for s in (False, True)]


@pytest.mark.parametrize("rows", [1, 7, 8, 9, 384])
@pytest.mark.parametrize("prior,post", CASES, ids=[f"{p}-{'sphere' if s else 'gauss'}" for p, s in CASES])
def test_kernels_match_autograd_in_every_mode(dev, prior, post, rows):
    mode, sprior = PRIORS[prior]
    for E in (32, 12):
        t = 16 if rows == 384 else rows
        use_ar1 = rows >= 2
        use_regu = mode != K.PRIOR_NONE
        d, keep = _inputs(dev, rows, t, E, seed=11 + rows + E)
        A, S, zc = d["pred"].shape[1], 37, 40
        kw = dict(prior=prior, post=post, t=t, E=E, use_ar1=use_ar1, use_regu=use_regu)
        w32, w64 = _formulas(d, dtype=torch.float32, **kw), _formulas(d, dtype=torch.float64, **kw)
        pw = 2 * E if mode == K.PRIOR_LEARNED else E
        ph = d["ph"][:, :pw].contiguous() if mode != K.PRIOR_NONE else None
        modes = dict(prior_mode=mode, prior_fixed_logvar=FIXED_LV, sphere_prior=sprior, embedding_norm=NORM)
        # ---- embed: z (projected or not) beside the self observation; nothing else is touched
        x = torch.randn(rows, 64, device=dev)
        ain = torch.full((rows, zc + E + 3), float("nan"), device=dev)
        cin = torch.full((rows, zc + E + 3), float("nan"), device=dev)
        K.vae_embed_modes(d["zh"], x, ain, rows=rows, embedding_size=E, self_obs_size=S, z_col=zc, eps=d["eps"], cin=cin, clamp=True, clamp_max=CLAMP_MAX,
                    sphere_posterior=post, embedding_norm=NORM)
        assert torch.equal(ain[:, :S], x[:, :S]) and torch.equal(cin[:, :S], x[:, :S])
        assert torch.isnan(ain[:, S:zc]).all() and torch.isnan(ain[:, zc + E:]).all() and torch.isnan(cin[:, S:]).all()
        _bound(ain[:, zc:zc + E], w32["z"], w64["z"], slice(None), 2e-6, f"z {prior} post={post} rows={rows} E={E}", post)
        if post and rows > ZERO_ROW:
            assert (ain[ZERO_ROW, zc:zc + E] == 0).all()                      # z = 0 projects to 0 / 1e-8 = 0
        K.vae_embed_modes(d["zh"], x, ain, rows=rows, embedding_size=E, self_obs_size=S, z_col=zc, eps=None, sphere_posterior=post, embedding_norm=NORM)
        zt = _formulas(d, dtype=torch.float32, test_mode=True, **kw)["z"]     # flags.test: z = mu, projected after the replacement
        zt64 = _formulas(d, dtype=torch.float64, test_mode=True, **kw)["z"]
        if post:
            _bound(ain[:, zc:zc + E], zt, zt64, slice(None), 2e-6, "z (test mode)", True)
        else:
            assert torch.equal(ain[:, zc:zc + E], d["zh"][:, :E])
        # ---- losses; one shape runs the block-stride loop (fewer blocks than groups of 8 rows)
        dmu = torch.full((rows, A), float("nan"), device=dev)
        partials = torch.full((5 if rows == 384 else 64, 8), float("nan"), device=dev)
        prog = d["prog"].contiguous() if use_ar1 else None
        K.vae_kin_loss_modes(d["pred"], d["gt"], d["zh"], ph, prog, dmu, partials, rows=rows, num_actions=A, embedding_size=E, horizon=t, use_ar1=use_ar1,
                       use_regu=use_regu, clamp=True, clamp_max=CLAMP_MAX, **modes)
        assert torch.isfinite(partials).all()
        s = partials.double().sum(0)
        n_err = max((rows // t) * (t - 1), 1)

        def close(a, b, b64, what, projected):
            tol = 2e-5 * max(abs(float(b)), 1e-6)
            if projected:
                margin = 4.0 * abs(float(b) - float(b64))
                print(f"{what}: base bound {tol:.3e}, 4 x fp32-vs-fp64 formula error {margin:.3e}, kernel error {abs(float(a) - float(b)):.3e}")
                tol = max(tol, margin)
            assert abs(float(a) - float(b)) <= tol, (what, float(a), float(b), tol)
        close(s[0] / rows, w32["act"], w64["act"], "action loss", False)
        close(s[1] / rows, w32["kld"], w64["kld"], f"KLD {prior}", sprior)
        if use_ar1:
            close(s[2] / n_err, w32["ar1"], w64["ar1"], "ar1", False)
        if use_regu:
            close((s[3] + s[4]) / (rows * E) * 0.001 + (s[5] + s[6]) / (rows * E) * 0.001, w32["regu"], w64["regu"], "regulariser", sprior)
        assert (dmu - w32["dpred"]).abs().max().item() <= 1e-6 * w32["dpred"].abs().max().item() + 1e-12
        # ---- head gradients
        dzh = torch.full((rows, 2 * E + 2), float("nan"), device=dev)
        dph = torch.full((rows, pw + 2), float("nan"), device=dev) if ph is not None else None
        K.vae_head_backward_modes(d["zh"], dzh, rows=rows, embedding_size=E, horizon=t, pheads=ph, dpheads=dph, eps=d["eps"], dz=d["dz"], progress=prog,
                            clamp=True, clamp_max=CLAMP_MAX, c_kl=0.01 / rows, c_ar1=(0.005 / n_err) if use_ar1 else 0.0,
                            c_regu=(0.005 * 0.001 / (rows * E)) if use_regu else 0.0, sphere_posterior=post, **modes)
        assert torch.isnan(dzh[:, 2 * E:]).all() and torch.isfinite(dzh[:, :2 * E]).all()
        _bound(dzh[:, :2 * E], w32["dzh"], w64["dzh"], keep, 3e-6, f"encoder heads {prior} post={post} rows={rows} E={E}", post)
        if rows > ZERO_ROW:
            got, want = dzh[ZERO_ROW, :2 * E], w32["dzh"][ZERO_ROW]
            assert torch.isfinite(got).all()
            if post:                                                          # autograd's g / 1e-8 there, compared relatively
                assert want[:E].abs().max() > 1e3
                assert ((got[:E] - want[:E]).abs() <= 1e-5 * want[:E].abs().max()).all(), (got[:E], want[:E])
                assert ((got[E:] - want[E:]).abs() <= 3e-6 * w32["dzh"][keep].abs().max() + 1e-10).all()
            else:
                assert ((got - want).abs() <= 3e-6 * w32["dzh"][keep].abs().max() + 1e-10).all()
        if ph is not None:
            assert torch.isnan(dph[:, pw:]).all()
            _bound(dph[:, :pw], w32["dph"], w64["dph"], slice(None), 3e-6, f"prior heads {prior} rows={rows} E={E}", sprior)
        outside = (d["zh"][:, E:] < -5) | (d["zh"][:, E:] > CLAMP_MAX)
        assert (dzh[:, E:2 * E][outside] == 0).all()                          # clamp mask


def test_launchers_reject_what_a_mode_cannot_run(dev):
    d, _ = _inputs(dev, 16, 8, 32, seed=2)
    dmu, partials, dzh = torch.empty(16, 69, device=dev), torch.zeros(8, 8, device=dev), torch.empty(16, 64, device=dev)
    base = dict(rows=16, num_actions=69, embedding_size=32, horizon=8)
    with pytest.raises(Exception, match="prior heads"):                       # a learned / fixed prior without its heads
        K.vae_kin_loss_modes(d["pred"], d["gt"], d["zh"], None, d["prog"], dmu, partials, prior_mode=K.PRIOR_FIXED, **base)
    with pytest.raises(Exception, match="regulariser"):
        K.vae_kin_loss_modes(d["pred"], d["gt"], d["zh"], None, d["prog"], dmu, partials, prior_mode=K.PRIOR_NONE, use_regu=True, **base)
    with pytest.raises(Exception, match="prior_mode"):
        K.vae_kin_loss_modes(d["pred"], d["gt"], d["zh"], d["ph"], d["prog"], dmu, partials, prior_mode=3, **base)
    with pytest.raises(Exception, match="strides"):                           # learned heads are 2E wide
        K.vae_kin_loss_modes(d["pred"], d["gt"], d["zh"], d["ph"][:, :32].contiguous(), d["prog"], dmu, partials, **base)
    with pytest.raises(Exception, match="embedding_norm"):
        K.vae_head_backward_modes(d["zh"], dzh, rows=16, embedding_size=32, eps=d["eps"], dz=d["dz"], sphere_posterior=True, embedding_norm=0.0)
    with pytest.raises(Exception, match="embedding_norm"):
        K.vae_embed_modes(d["zh"], torch.zeros(16, 64, device=dev), torch.zeros(16, 80, device=dev), rows=16, embedding_size=32, self_obs_size=37, z_col=40,
                    sphere_posterior=True, embedding_norm=-1.0)
    with pytest.raises(Exception, match="regulariser"):
        K.vae_head_backward_modes(d["zh"], dzh, rows=16, embedding_size=32, eps=d["eps"], dz=d["dz"], prior_mode=K.PRIOR_NONE, c_regu=1e-6)


def test_defaults_are_the_learned_gaussian_form_bit_for_bit(dev):
    """The wrappers under their recorded signatures (the calls of tests/test_vae_head_gpu.py), the ``*_modes`` wrappers with no mode
    given and with the default modes spelled out: one result, bit for bit."""
    rows, t, E, A, S, zc = 384, 16, 32, 69, 358, 360
    d, _ = _inputs(dev, rows, t, E, seed=3)
    explicit = dict(prior_mode=K.PRIOR_LEARNED, prior_fixed_logvar=0.0, sphere_prior=False, embedding_norm=1.0)
    x = torch.randn(rows, 960, device=dev)
    outs = []
    for embed, kin, bwd, kw, pkw in ((K.vae_embed, K.vae_kin_loss, K.vae_head_backward, {}, {}),
                                     (K.vae_embed_modes, K.vae_kin_loss_modes, K.vae_head_backward_modes, {}, {}),
                                     (K.vae_embed_modes, K.vae_kin_loss_modes, K.vae_head_backward_modes, explicit, {"sphere_posterior": False})):
        ain, cin = torch.full((rows, 392), float("nan"), device=dev), torch.full((rows, 392), float("nan"), device=dev)
        embed(d["zh"], x, ain, rows=rows, embedding_size=E, self_obs_size=S, z_col=zc, eps=d["eps"], cin=cin, clamp=True, clamp_max=2.0,
              **(dict(pkw, embedding_norm=1.0) if pkw else {}))
        dmu, partials = torch.full((rows, A), float("nan"), device=dev), torch.zeros(64, 8, device=dev)
        kin(d["pred"], d["gt"], d["zh"], d["ph"], d["prog"], dmu, partials, rows=rows, num_actions=A, embedding_size=E, horizon=t, use_ar1=True,
            use_regu=True, **kw)
        dzh, dph = torch.full((rows, 2 * E), float("nan"), device=dev), torch.full((rows, 2 * E), float("nan"), device=dev)
        bwd(d["zh"], dzh, rows=rows, embedding_size=E, horizon=t, pheads=d["ph"], dpheads=dph, eps=d["eps"], dz=d["dz"], progress=d["prog"],
            c_kl=0.01 / rows, c_ar1=0.005 / 360, c_regu=0.005 * 0.001 / (rows * E), **kw, **pkw)
        outs.append((ain, cin, dmu, partials, dzh, dph))
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))
    # and they are the learned-prior formulas
    w = _formulas(d, prior="learned", post=False, t=t, E=E, use_ar1=True, use_regu=True, dtype=torch.float32)
    assert (outs[0][4] - w["dzh"]).abs().max().item() <= 3e-6 * w["dzh"].abs().max().item() + 1e-10


def test_project_kernel_is_project_to_norm(dev):
    for rows, E in ((1, 32), (9, 12), (130, 32)):
        g = torch.Generator().manual_seed(rows)
        a, b = torch.randn(rows, E, generator=g).to(dev), torch.randn(rows, E, generator=g).to(dev)
        out = torch.full((rows, E + 3), float("nan"), device=dev)
        K.vae_project(a, out, rows=rows, cols=E, norm=1.0, b=b)
        want = VM.project_to_norm(b + a, 1)
        assert (out[:, :E] - want).abs().max().item() <= 2e-6 and torch.isnan(out[:, E:]).all()
        K.vae_project(a, out, rows=rows, cols=E, norm=NORM)
        assert (out[:, :E] - VM.project_to_norm(a, NORM)).abs().max().item() <= 2e-6 * NORM


# --------------------------------------------------------------------------------------------------------------------------- the agent
def rel_close(a, b, tol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    scale = b.abs().max().item() + 1e-12
    err = (a - b).abs().max().item()
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _restatement(variant):
    v = configs.VAE_VARIANTS[variant]
    return VM.VariantNetZ(use_vae_prior=v.get("use_vae_prior", True), use_vae_fixed_prior=v.get("use_vae_fixed_prior", False),
                          use_vae_sphere_prior=v.get("use_vae_sphere_prior", False), use_vae_sphere_posterior=v.get("use_vae_sphere_posterior", False),
                          vae_prior_fixed_logvar=v.get("vae_prior_fixed_logvar", 0), embedding_norm=v.get("embedding_norm", 1))


@pytest.mark.parametrize("variant,regu", [("none", False), ("fixed", True), ("fixed_sphere", False), ("sphere_post", False),
                                          ("none_sphere_post", False), ("fixed_sphere_post", True)])
def test_optimize_kin_matches_the_restatement(dev, variant, regu):
    torch.manual_seed(5)
    agent, _ = configs.make_agent("cfg3_small", device=str(dev), seed=5, env_overrides=configs.vae_variant_env(variant, use_vae_prior_regu=regu))
    agent.init_tensors()
    ref = _restatement(variant)
    agent.model.load_state_dict(ref.state_dict_ref())
    t, mb = agent.horizon_length, agent.minibatch_size
    obs = torch.randn(mb, 934).clamp(-5, 5)
    gt = (0.4 * torch.randn(mb, 69)).clamp(-1, 1)
    prog = (torch.randint(0, 40, (mb // t, 1)) + torch.arange(t)[None, :]).reshape(-1, 1)
    prog[3 * t + 5:3 * t + t] = torch.arange(t - 5)[:, None]                  # an episode seam inside sequence 3
    noise = torch.randn(mb, 32)
    info_ref = VM.optimize_kin(ref, obs, gt, prog, noise, t, use_vae_prior_regu=regu)
    ws = agent.model.workspace(mb, train=True)
    ws["x"].zero_()
    ws["x"][:, :934] = obs.to(dev)
    agent.z_noise_provider = lambda m: noise.to(dev)
    agent.set_train()
    if not ref.has_prior:
        assert "fwd_prior" not in ws["G"] and "bwd_prior" not in ws["G"]       # no prior: no plans to launch
    info = agent._optimize_kin(ws, mb, {"gt_action": gt.to(dev), "progress_buf": prog.to(dev)})
    for k in ("kin_action_loss", "kin_KLD", "kin_ar1", "kin_loss") + (("kin_prior_regu",) if regu else ()):
        np.testing.assert_allclose(info[k].item(), info_ref[k].item(), rtol=2e-5, err_msg=k)
    grads = agent.model.net.gradients()
    names = {"a2c_network." + n for n, _ in ref.named_parameters()} - {"a2c_network.sigma"}
    assert set(grads) == names, set(grads) ^ names                            # parameters a mode does not have are absent
    total_sq = 0.0
    for name, p in ref.named_parameters():
        if name == "sigma":
            continue
        if p.grad is None:
            assert torch.count_nonzero(grads["a2c_network." + name]) == 0, f"{name} must get no gradient in kin mode"
            continue
        rel_close(grads["a2c_network." + name], p.grad, 3e-4, f"grad {name}")
        total_sq += p.grad.double().pow(2).sum().item()
    np.testing.assert_allclose(info["grad_norm"].item(), total_sq ** 0.5, rtol=1e-4)


# ----------------------------------------------------------------------------------------------------------------------------- the env
@pytest.mark.parametrize("variant", ["fixed", "none", "sphere_post", "fixed_sphere_post"])
def test_compute_z_actions_matches_the_restatement(dev, variant):
    from pulse_amd.env.humanoid_z import HumanoidImZ
    from pulse_amd.env.sim import RecordedMotion, RecordedRollout, RecordedSim
    torch.manual_seed(9)
    n = 130
    rollout = RecordedRollout(n, 3, seed=21).to(dev)
    sim = RecordedSim(rollout)
    env = dict(configs.ENV_IM, embedding_size=32, **configs.vae_variant_env(variant))
    task = HumanoidImZ({"env": env}, sim, RecordedMotion(rollout, sim), device=dev)
    ref = _restatement(variant)
    rm, rv = torch.randn(934).double() * 0.3, (torch.rand(934) + 0.5).double()
    task.initialize_z_models({"model": ref.state_dict_ref(), "running_mean_std": {"running_mean": rm, "running_var": rv}}, configs.NETWORK_Z)
    task.reset()
    if ref.has_prior and not ref.use_vae_prior:                               # fixed prior: its mean is not added, so its plan must not run
        def boom():
            raise AssertionError("the prior plan ran under a fixed prior")
        task._z_graph["fwd_prior"] = type("P", (), {"run": staticmethod(boom)})()
    if not ref.has_prior:
        assert "fwd_prior" not in task._z_graph
    az = 0.5 * torch.randn(n, 32)
    act = task.compute_z_actions(az.to(dev)).clone()
    want = VM.compute_z_actions(ref, task.obs_buf.cpu(), rm, rv, az)
    rel_close(act, want, 5e-5, "z -> action")
    if ref.use_vae_sphere_posterior:                                          # radius 1, not the model's embedding_norm (2)
        zc = task._z_net.z_col
        zn = task._z_graph["g"].act_bufs["ain"][:, zc:zc + 32].norm(dim=-1)
        assert (zn - 1.0).abs().max().item() <= 1e-5
    task.step(az.to(dev))
    assert torch.isfinite(task.obs_buf).all()


def test_downstream_task_reads_the_variant_from_its_env_dict(dev):
    """HumanoidSpeedZ (env_pulse_amp.yaml) on a frozen model without a prior and with the sphere posterior: one epoch of the reader policy."""
    agent, _ = configs.make_agent("speed_z_small", device=str(dev), seed=5, env_overrides=configs.vae_variant_env("none_sphere_post"))
    task = agent.vec_env.env.task
    znet = task._z_net
    assert znet.prior_mode == K.PRIOR_NONE and znet.use_vae_sphere_posterior and "fwd_prior" not in task._z_graph
    assert not any(k.startswith("a2c_network.z_prior") for k in znet.state_dict())
    info = agent.train_epoch()
    assert all(torch.isfinite(torch.as_tensor(x)).all() for x in info["actor_loss"])
    zn = task._z_graph["g"].act_bufs["ain"][:, znet.z_col:znet.z_col + 32].norm(dim=-1)
    assert (zn - 1.0).abs().max().item() <= 1e-5                            # the decoder saw latents of radius 1


# -------------------------------------------------------------------------------------------------------------------------- epochs
@pytest.mark.parametrize("name,variant", [("cfg3_small", "fixed_sphere_post"), ("cfg3_small", "none"), ("cfg3_ppo_small", "sphere_post")])
def test_variant_agents_run_epochs_and_learn(dev, name, variant):
    agent, _ = configs.make_agent(name, device=str(dev), seed=3, env_overrides=configs.vae_variant_env(variant))
    before = agent.model.flat.clone()
    first = None
    for e in range(3):
        info = agent.train_epoch()
        key = "kin_loss" if "kin_loss" in info else "critic_loss"
        val = torch.stack(info[key]).mean().item()
        assert np.isfinite(val)
        first = val if first is None else first
    assert val < first, f"{key} should decrease over 3 epochs ({first} -> {val})"
    assert not torch.equal(before, agent.model.flat)
    eb = agent.experience_buffer
    assert torch.isfinite(eb.tensor_dict["mus"]).all() and torch.isfinite(eb.tensor_dict["values"]).all()
    if key == "kin_loss":
        assert np.isfinite(torch.stack(info["kin_KLD"]).mean().item())
        has_prior = any(k.startswith("a2c_network.z_prior") for k in agent.model.state_dict())
        assert has_prior == (variant != "none")
