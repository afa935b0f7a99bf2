"""Generate tests/golden/prior_sampling.npz: the reference's own form_embedding with ``flags.debug`` on -- the latent drawn from the prior.

    python tools/gen_golden_prior_sampling.py [--out DIR]

Needs the reference tree (oracle/refload.py reads its methods at run time; nothing of its text is kept here).  Networks, inputs and the
reference stubs are those of tools/gen_golden_vae_variants.py (``make_net`` / ``inputs`` / ``reference_net`` / ``reference_flags``); the
fixture holds OUTPUTS only, plus the float64 sums of the inputs.

Cases: prior in {learned, fixed, fixed_sphere, none} x posterior in {gauss, sphere}
  z/<prior>/<post>           AMPZBuilder.Network.form_embedding under flags.debug (amp_network_z_builder.py:101-119)
  z_post/<prior>/<post>      the same call, same seed, flags.debug off: the posterior's latent, which the prior's must not equal
  prior/<prior>/<post>/{mu, logvar}     compute_prior (:226-241); not for none
  heads/<prior>/{mu, logvar}            the raw z_prior_mu / z_prior_logvar outputs (logvar under the learned prior only): what the kernel reads
  eps                        the noise of the prior's draw

The reference draws that noise itself (reparameterize's randn_like, :245-248; :116 without a prior), after the posterior's own draw.  It is
recovered by re-seeding and drawing the same shapes in the same order, and the fixture is written only if
prior_mu + eps * exp(0.5 prior_logvar) -- projected where the mode says so -- reproduces the reference's z bit for bit.
"""
import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden_vae_variants as GV  # noqa: E402
import prior_sampling_model as PM  # noqa: E402
import vae_variants_model as VM  # noqa: E402

DRAW_SEED = 4409
# make_net scales z_prior_logvar's weight by 40 (its bias is zero); on the 40 input rows that puts the raw log-variance on both sides of the
# clamp range [-5, var_clamp_max] already -- check_conditions holds it to that.  A larger factor here would widen it further.
PRIOR_LOGVAR_SCALE = 1.0
MAX_BYTES = GV.MAX_BYTES
PRIORS, POSTS = list(VM.MODES), list(GV.POSTS)


def make_net(prior, post):
    net = GV.make_net(prior, post)
    if PRIOR_LOGVAR_SCALE != 1.0 and hasattr(net, "z_prior_logvar"):
        with torch.no_grad():
            net.z_prior_logvar.weight.mul_(PRIOR_LOGVAR_SCALE)
            net.z_prior_logvar.bias.mul_(PRIOR_LOGVAR_SCALE)
    return net


def inputs():
    return GV.inputs()


def input_sums(d):
    out = {f"sum_{k}": v.double().sum() for k, v in d.items()}
    out["sum_params"] = sum(p.detach().double().sum() for p in make_net("learned", "gauss").parameters())
    return out


def recovered_noise(rows, E):
    """(the posterior's draw, the prior's draw): the two randn_like calls of one form_embedding under flags.debug, in their order."""
    torch.manual_seed(DRAW_SEED)
    like = torch.empty(rows, E)
    return torch.randn_like(like), torch.randn_like(like)


def reference_case(prior, post, d):
    net = make_net(prior, post)
    ref = GV.reference_net(net).train()
    flags = GV.reference_flags()
    obs = d["obs"]
    batch = {"obs": obs}                                     # no 'z_noise': the reference draws the posterior's noise itself
    out = {}
    with torch.no_grad():
        torch.manual_seed(DRAW_SEED)
        z_post, _ = ref.form_embedding(ref.z_mlp(obs), batch)
        flags.debug = True
        try:
            torch.manual_seed(DRAW_SEED)
            with contextlib.redirect_stdout(io.StringIO()):  # (the branch prints a progress line)
                z, _ = ref.form_embedding(ref.z_mlp(obs), batch)
        finally:
            flags.debug = False
        assert flags.test is False and flags.trigger_input is False
        k = f"{prior}/{post}"
        out.update({f"z/{k}": z.clone(), f"z_post/{k}": z_post.clone()})
        mu = lv = None
        if prior != "none":
            pm, pv = ref.compute_prior(batch)
            out.update({f"prior/{k}/mu": pm, f"prior/{k}/logvar": pv})
            lat = ref.z_prior(obs[:, :ref.self_obs_size])
            mu = ref.z_prior_mu(lat)
            out[f"heads/{prior}/mu"] = mu
            if prior == "learned":
                lv = ref.z_prior_logvar(lat)
                out[f"heads/{prior}/logvar"] = lv
        # ---- the noise, recovered; nothing is written unless it reproduces the reference's z exactly
        _, eps = recovered_noise(*z.shape)
        again = PM.z_from_prior_heads(mu, lv, eps, **PM.net_modes(net))
        assert torch.equal(again, z), f"{k}: the recovered noise does not reproduce the reference's z (max diff {(again - z).abs().max():.3e})"
        if prior != "none":                                  # and by the reference's own returned prior, spelled as the issue states it
            direct = pm + eps * torch.exp(0.5 * pv)
            assert torch.equal(VM.project_to_norm(direct, GV.NORM) if GV.POSTS[post] else direct, z), k
        out["eps"] = eps
    return out


def generate():
    d = inputs()
    out = {}
    for post in POSTS:
        for prior in PRIORS:
            case = reference_case(prior, post, d)
            if "eps" in out:
                assert torch.equal(out["eps"], case["eps"])
            out.update(case)
    check_conditions(out)
    out.update(input_sums(d))
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}


def check_conditions(out):
    """The conditions that keep the fixture from hiding a failure; AssertionError otherwise.  Takes tensors or arrays."""
    t = lambda k: torch.as_tensor(out[k])
    for prior in PRIORS:
        for post in POSTS:
            z, zp = t(f"z/{prior}/{post}"), t(f"z_post/{prior}/{post}")
            assert ((z != zp).any(dim=-1)).all(), f"{prior}/{post}: a row's prior z equals its posterior z"
            if GV.POSTS[post]:
                assert ((z.double().norm(dim=-1) - GV.NORM).abs() <= 1e-6).all(), f"{prior}/{post}: a sphere-posterior row is off the sphere"
    lv = t("heads/learned/logvar")
    assert (lv < -5).any() and (lv > VM_CLAMP_MAX).any() and ((lv > -5) & (lv < VM_CLAMP_MAX)).any(), \
        f"the raw prior log-variance must lie on both sides of [-5, {VM_CLAMP_MAX}]: [{lv.min():.2f}, {lv.max():.2f}]"
    for post in POSTS:
        clamped = t(f"prior/learned/{post}/logvar")
        assert (clamped == -5).any() and (clamped == VM_CLAMP_MAX).any()
        a, b = t(f"prior/fixed/{post}/mu"), t(f"prior/fixed_sphere/{post}/mu")
        assert ((a != b).any(dim=-1)).all(), "the sphere-prior mean must differ from the unprojected mean in every row"
        assert (t(f"prior/fixed/{post}/logvar") == GV.FIXED_LOGVAR).all()


VM_CLAMP_MAX = 2.0          # OracleNetZ.var_clamp_max, the vae_var_clamp_max of env_im_vae.yaml


def load(path=None):
    z = np.load(path or os.path.join(ROOT, "tests", "golden", "prior_sampling.npz"))
    return {k: z[k] for k in z.files}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    path = os.path.join(a.out, "prior_sampling.npz")
    np.savez_compressed(path, **generate())
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= MAX_BYTES, f"{size} bytes: the fixture must stay under {MAX_BYTES}"


if __name__ == "__main__":
    main()
