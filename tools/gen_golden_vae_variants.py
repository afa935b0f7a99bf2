"""Generate tests/golden/vae_variants.npz: the reference's own method bodies on the PULSE VAE's prior / posterior variants.

    python tools/gen_golden_vae_variants.py [--out DIR]

Needs the reference tree (oracle/refload.py reads its methods at run time; nothing of its text is kept here).  The committed fixture holds
OUTPUTS only, written by
  AMPZBuilder.Network.form_embedding / compute_prior / eval_actor   refload.learning_methods()["ampz_net"]
  AMPAgent._optimize_kin                                            refload.learning_methods()["agent"]
  load_z_decoder + HumanoidZ.compute_z_actions                      refload.network_loader_functions()
run on stub objects that carry a small tests/vae_variants_model.VariantNetZ's modules; inputs and weights are redrawn from the seed by
``make_net`` / ``inputs`` (the tests call them too) and the fixture carries their float64 sums, so other draws are noticed.

Cases: prior in {learned, fixed, fixed_sphere, none} x posterior in {gauss, sphere}
  net/<prior>/<post>/<train|test>/{z, mu, vae_mu, vae_log_var}         form_embedding + eval_actor, flags.test off / on
  prior/<prior>/<post>/{mu, logvar}                                    compute_prior (not for none); prior/both/.. = both switches on
  kin/<prior>/<post>/<ar1|noar1>/<regu|noregu>/{info, grads}           _optimize_kin: [action loss, KLD, ar1, regu, kin loss] and every
                                                                       parameter gradient, flattened in named_parameters() order
                                                                       (regu only where a prior exists)
  env/<prior>/<post>/actions                                           compute_z_actions
embedding_norm is 1.7 and vae_prior_fixed_logvar -0.6, so neither can be mistaken for a default; the env's sphere posterior uses radius 1.
"""
import argparse
import copy
import os
import sys
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import vae_variants_model as VM  # noqa: E402

SEED = 9127
SIZES = dict(self_obs_size=10, task_obs_size=9, actions_num=5, units=(12, 10), task_units=(11, 9), embedding_size=6)
NORM, FIXED_LOGVAR = 1.7, -0.6
HORIZON, NSEQ = 8, 5
POSTS = {"gauss": False, "sphere": True}
MAX_BYTES = 1024 * 1024


def make_net(prior, post, **extra):
    """The small network of a case: the same draws whatever the mode; log-variance weights scaled so the clamp acts on some entries."""
    torch.manual_seed(SEED)
    kw = dict(VM.MODES[prior] if prior != "both" else dict(use_vae_prior=True, use_vae_fixed_prior=True, use_vae_sphere_prior=True))
    net = VM.VariantNetZ(use_vae_sphere_posterior=POSTS[post], vae_prior_fixed_logvar=FIXED_LOGVAR, embedding_norm=NORM, **kw, **SIZES, **extra)
    with torch.no_grad():
        net.z_logvar.weight.mul_(40.0)
        if hasattr(net, "z_prior_logvar"):
            net.z_prior_logvar.weight.mul_(40.0)
    return net


def inputs():
    g = torch.Generator().manual_seed(SEED + 1)
    mb, E, A = HORIZON * NSEQ, SIZES["embedding_size"], SIZES["actions_num"]
    width = SIZES["self_obs_size"] + SIZES["task_obs_size"]
    prog = torch.arange(HORIZON).repeat(NSEQ, 1) + torch.randint(0, 50, (NSEQ, 1), generator=g)
    prog[2, 4:] = torch.arange(HORIZON - 4)                                  # an episode seam inside a sequence
    prog[4, :] = torch.arange(HORIZON)                                       # a sequence that starts at progress 0
    return {"obs": torch.randn(mb, width, generator=g).clamp(-5, 5), "noise": torch.randn(mb, E, generator=g),
            "gt": (0.4 * torch.randn(mb, A, generator=g)).clamp(-1, 1), "prog": prog.reshape(-1).float(),
            "obs_buf": torch.randn(mb, width, generator=g) * 2.0, "running_mean": (torch.randn(width, generator=g) * 0.3).double(),
            "running_var": (torch.rand(width, generator=g) + 0.5).double(), "action_z": 0.5 * torch.randn(mb, E, generator=g)}


def input_sums(d):
    out = {f"sum_{k}": v.double().sum() for k, v in d.items()}
    out["sum_params"] = sum(p.detach().double().sum() for p in make_net("learned", "gauss").parameters())
    return out


def kin_cases():
    for prior in VM.MODES:
        for post in POSTS:
            for ar1 in (True, False):
                for regu in ((False, True) if prior != "none" else (False,)):
                    yield prior, post, ar1, regu


def kin_key(prior, post, ar1, regu):
    return f"kin/{prior}/{post}/{'ar1' if ar1 else 'noar1'}/{'regu' if regu else 'noregu'}"


def info_vector(info):
    z = torch.zeros(())
    return torch.stack([info["kin_action_loss"], info["kin_KLD"], info.get("kin_ar1", z), info.get("kin_prior_regu", z), info["kin_loss"]]).detach()


def flat_grads(net):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for n, p in net.named_parameters() if n != "sigma"])


# ---------------------------------------------------------------------------------------------------------------- the reference on stubs
def _bind(obj, fns):
    for k, f in fns.items():
        setattr(obj, k, types.MethodType(f, obj))
    return obj


def reference_net(net):
    """A copy of ``net``'s modules that runs the reference's AMPZBuilder.Network methods."""
    from oracle import refload
    ref = _bind(copy.deepcopy(net), refload.learning_methods()["ampz_net"])
    for k, v in dict(actor_cnn=nn.Sequential(), critic_cnn=nn.Sequential(), has_rnn=False, proj_norm=True, z_type="vae",
                     use_vae_clamped_prior=net.use_vae_clamped_prior, vae_var_clamp_max=net.var_clamp_max, z_all=False, is_discrete=False,
                     is_multi_discrete=False, is_continuous=True, mu_act=nn.Identity(), sigma_act=nn.Identity(), value_act=nn.Identity(),
                     space_config={"fixed_sigma": True}, z_noise=None).items():
        setattr(ref, k, v)
    return ref                      # (the six switches are attributes of VariantNetZ under the reference's names already)


def reference_flags():
    from oracle import refload
    return refload.learning_methods()["ampz_net"]["form_embedding"].__globals__["flags"]


def reference_net_outputs(prior, post, d):
    out = {}
    ref = reference_net(make_net(prior, post)).train()
    flags = reference_flags()
    for mode in ("train", "test"):
        flags.test = mode == "test"
        try:
            batch = {"obs": d["obs"], "z_noise": d["noise"]}
            z, _ = ref.form_embedding(ref.z_mlp(d["obs"]), batch)
            mu, _, extra = ref.eval_actor(batch, return_extra=True)
        finally:
            flags.test = False
        out.update({f"net/{prior}/{post}/{mode}/z": z, f"net/{prior}/{post}/{mode}/mu": mu,
                    f"net/{prior}/{post}/{mode}/vae_mu": extra["vae_mu"], f"net/{prior}/{post}/{mode}/vae_log_var": extra["vae_log_var"]})
    if prior != "none":
        pm, pv = ref.compute_prior({"obs": d["obs"]})
        out.update({f"prior/{prior}/{post}/mu": pm, f"prior/{prior}/{post}/logvar": pv})
    return out


def reference_kin(prior, post, ar1, regu, d):
    from oracle import refload
    ref = reference_net(make_net(prior, post)).train()
    mb, A = d["obs"].shape[0], SIZES["actions_num"]
    env = types.SimpleNamespace(distill=True, z_type="vae", use_ar1_prior=ar1, use_vae_prior_regu=regu, kld_coefficient=0.01, ar1_coefficient=0.005,
                                kld_anneal=False, kld_coefficient_min=0.001, use_vae_prior=ref.use_vae_prior, use_vae_fixed_prior=ref.use_vae_fixed_prior)
    agent = types.SimpleNamespace(vec_env=types.SimpleNamespace(env=types.SimpleNamespace(task=env)),
                                  model=types.SimpleNamespace(a2c_network=ref, parameters=ref.parameters), minibatch_size=mb,
                                  horizon_length=HORIZON, epoch_num=10, grad_norm=1e9, kin_optimizer=torch.optim.SGD(ref.parameters(), 0.0),
                                  kin_dict_info={"gt_action": ((mb, A), (mb, A)), "progress_buf": ((mb,), (mb, 1))})
    _bind(agent, refload.learning_methods()["agent"])
    info = agent._optimize_kin({"obs": d["obs"], "z_noise": d["noise"], "kin_dict": torch.cat([d["gt"], d["prog"].unsqueeze(-1)], dim=-1)})
    k = kin_key(prior, post, ar1, regu)
    return {k + "/info": info_vector(info), k + "/grads": flat_grads(ref)}


def reference_env(prior, post, d):
    from oracle import refload
    f = refload.network_loader_functions()
    net = make_net(prior, post)
    ck = {"model": net.state_dict_ref()}
    dec = f["load_z_decoder"](ck, activation="silu", z_type="vae", device="cpu")
    enc = f["load_z_encoder"](ck, activation="silu", z_type="vae", device="cpu")
    stub = types.SimpleNamespace(get_self_obs_size=lambda: SIZES["self_obs_size"], obs_buf=d["obs_buf"], running_mean=d["running_mean"],
                                 running_var=d["running_var"], distill_z_type="vae", use_vae_prior=net.use_vae_prior,
                                 use_vae_sphere_posterior=net.use_vae_sphere_posterior, cfg={"env": {"embedding_norm": NORM}}, z_all=False,
                                 decoder=dec, encoder=enc, is_discrete=False, embedding_size_distill=SIZES["embedding_size"])
    return {f"env/{prior}/{post}/actions": f["compute_z_actions"](stub, d["action_z"].clone())}


def generate():
    d = inputs()
    out = {}
    for post in POSTS:
        for prior in list(VM.MODES) + ["both"]:
            if prior == "both":
                pm, pv = reference_net(make_net("both", post)).compute_prior({"obs": d["obs"]})
                out.update({f"prior/both/{post}/mu": pm, f"prior/both/{post}/logvar": pv})
                continue
            out.update(reference_net_outputs(prior, post, d))
            out.update(reference_env(prior, post, d))
    for case in kin_cases():
        out.update(reference_kin(*case, d))
    check_conditions(out)
    out.update(input_sums(d))
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}


def check_conditions(out):
    """The conditions that keep the fixture from hiding a failure; AssertionError otherwise."""
    lv = out["net/learned/gauss/train/vae_log_var"]
    assert (lv == -5).any() and (lv == 2).any() and ((lv > -5) & (lv < 2)).any(), "the clamp must act on some log-variances and not on others"
    for post in POSTS:
        assert not torch.equal(out[f"prior/fixed/{post}/mu"], out[f"prior/fixed_sphere/{post}/mu"])
        assert torch.equal(out[f"prior/both/{post}/mu"], out[f"prior/learned/{post}/mu"]), "both switches: the learned branch wins"
        assert torch.equal(out[f"prior/both/{post}/logvar"], out[f"prior/learned/{post}/logvar"])
        assert (out[f"prior/fixed/{post}/logvar"] == FIXED_LOGVAR).all()
        assert torch.equal(out[f"env/fixed/{post}/actions"], out[f"env/none/{post}/actions"]), "under a fixed prior the mean is not added"
        assert not torch.equal(out[f"env/learned/{post}/actions"], out[f"env/none/{post}/actions"])
    for prior in VM.MODES:
        for mode in ("train", "test"):
            a, b = out[f"net/{prior}/gauss/{mode}/z"], out[f"net/{prior}/sphere/{mode}/z"]
            assert not torch.equal(a, b) and torch.allclose(b.norm(dim=-1), torch.full((b.shape[0],), NORM), rtol=1e-5)
            assert torch.equal(out[f"net/{prior}/gauss/{mode}/vae_mu"], out[f"net/{prior}/sphere/{mode}/vae_mu"]), "the heads stay unprojected"
        assert torch.equal(out[f"net/{prior}/gauss/test/z"], out[f"net/{prior}/gauss/test/vae_mu"])
    klds = {p: float(out[kin_key(p, "gauss", True, False) + "/info"][1]) for p in VM.MODES}
    assert len(set(klds.values())) == 4, f"the four priors must give four KL values: {klds}"


def load(path=None):
    z = np.load(path or os.path.join(ROOT, "tests", "golden", "vae_variants.npz"))
    return {k: z[k] for k in z.files}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    path = os.path.join(a.out, "vae_variants.npz")
    np.savez_compressed(path, **generate())
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= MAX_BYTES, f"{size} bytes: the fixture must stay under {MAX_BYTES}"


if __name__ == "__main__":
    main()
