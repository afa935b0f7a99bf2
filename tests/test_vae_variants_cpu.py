"""CPU: the PULSE VAE's prior / posterior variants (no prior, fixed prior, sphere prior, sphere posterior).

  * tests/vae_variants_model.py (the plain-torch restatement the GPU tests compare against) equals tests/golden/vae_variants.npz -- outputs
    of the reference's own method bodies -- bit for bit, for every combination the reference can run;
  * where the reference checkout is present, its method bodies reproduce the fixture key by key, and with both prior switches on the
    learned branch runs;
  * AMPZNetwork's state_dict has exactly the reference's key set and shapes per mode, and the reference's loaders accept it;
  * what is still not built raises by name without a device; the env keys are classified HONOURED and dicts that switch them on pass."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden_vae_variants as GV  # noqa: E402
import vae_variants_model as VM  # noqa: E402
from oracle import refload  # noqa: E402
from pulse_amd import configs  # noqa: E402
from pulse_amd.env import env_keys  # noqa: E402
from pulse_amd.learning.network_z import AMPZNetwork  # noqa: E402

PRIORS, POSTS = list(VM.MODES), list(GV.POSTS)


@pytest.fixture(scope="module")
def fx():
    return GV.load()


@pytest.fixture(scope="module")
def d():
    return GV.inputs()


def same(t, a):
    return np.array_equal(t.detach().numpy(), a)


def test_inputs_are_the_ones_the_fixture_was_made_from(fx, d):
    for k, v in GV.input_sums(d).items():
        assert float(v) == float(fx[k]), k


@pytest.mark.parametrize("post", POSTS)
@pytest.mark.parametrize("prior", PRIORS)
def test_restatement_network_equals_reference_outputs(fx, d, prior, post):
    net = GV.make_net(prior, post).train()
    for mode in ("train", "test"):
        net.test = mode == "test"
        z, _ = net.form_embedding(net.z_mlp(d["obs"]), d["noise"])
        mu, _, extra = net.eval_actor(d["obs"], d["noise"])
        k = f"net/{prior}/{post}/{mode}/"
        assert same(z, fx[k + "z"]) and same(mu, fx[k + "mu"]), k
        assert same(extra["vae_mu"], fx[k + "vae_mu"]) and same(extra["vae_log_var"], fx[k + "vae_log_var"]), k
    if prior == "none":
        assert not any(n.startswith("z_prior") for n, _ in net.named_parameters())
    else:
        pm, pv = net.compute_prior(d["obs"])
        assert same(pm, fx[f"prior/{prior}/{post}/mu"]) and same(pv, fx[f"prior/{prior}/{post}/logvar"])
        assert ("z_prior_logvar.weight" in dict(net.named_parameters())) == (prior == "learned")


@pytest.mark.parametrize("post", POSTS)
def test_both_prior_switches_take_the_learned_branch(fx, d, post):
    pm, pv = GV.make_net("both", post).compute_prior(d["obs"])
    assert same(pm, fx[f"prior/both/{post}/mu"]) and same(pv, fx[f"prior/both/{post}/logvar"])
    assert np.array_equal(fx[f"prior/both/{post}/mu"], fx[f"prior/learned/{post}/mu"])
    assert np.array_equal(fx[f"prior/both/{post}/logvar"], fx[f"prior/learned/{post}/logvar"])


@pytest.mark.parametrize("case", list(GV.kin_cases()), ids=lambda c: GV.kin_key(*c)[4:])
def test_restatement_kin_loss_equals_reference_method(fx, d, case):
    prior, post, ar1, regu = case
    net = GV.make_net(prior, post).train()
    info = VM.optimize_kin(net, d["obs"], d["gt"], d["prog"], d["noise"], GV.HORIZON, use_ar1_prior=ar1, use_vae_prior_regu=regu)
    k = GV.kin_key(*case)
    assert same(GV.info_vector(info), fx[k + "/info"]), (k, GV.info_vector(info), fx[k + "/info"])
    assert same(GV.flat_grads(net), fx[k + "/grads"]), k
    if prior == "fixed" and regu:                                # the constant log-variance counts in the reported regulariser
        assert float(fx[k + "/info"][3]) > 0.001 * GV.FIXED_LOGVAR ** 2


@pytest.mark.parametrize("post", POSTS)
@pytest.mark.parametrize("prior", PRIORS)
def test_restatement_env_actions_equal_reference_method(fx, d, prior, post):
    net = GV.make_net(prior, post)
    got = VM.compute_z_actions(net, d["obs_buf"], d["running_mean"], d["running_var"], d["action_z"])
    assert same(got, fx[f"env/{prior}/{post}/actions"])


@pytest.mark.skipif(not refload.available(), reason="reference checkout not present: the fixture stands in for it")
def test_reference_method_bodies_reproduce_the_fixture(fx):
    live = GV.generate()
    assert set(live) == set(fx)
    for k in sorted(fx):
        assert np.array_equal(live[k], fx[k]), k


# ------------------------------------------------------------------------------------------------------------------ the network's parameters
def _detail(prior, **extra):
    det = {"embedding_size": 32, "embedding_norm": 1, "z_type": "vae", "use_vae_clamped_prior": True, "vae_var_clamp_max": 2}
    det.update(VM.MODES[prior])
    det.update(extra)
    return det


def _network(prior, **extra):
    return AMPZNetwork(configs.NETWORK_Z, actions_num=69, self_obs_size=358, task_obs_size=576, task_obs_size_detail=_detail(prior, **extra), device="cpu")


@pytest.mark.parametrize("prior", PRIORS)
def test_state_dict_has_the_references_key_set_per_mode(prior):
    sd = _network(prior).state_dict()
    ref = VM.VariantNetZ(**VM.MODES[prior])
    want = ref.state_dict_ref()
    assert set(sd) == set(want), set(sd) ^ set(want)
    for k in want:
        assert tuple(sd[k].shape) == tuple(want[k].shape), k
    has = {k for k in sd if k.startswith("a2c_network.z_prior")}
    if prior == "none":
        assert not has
    else:
        assert ("a2c_network.z_prior_logvar.weight" in has) == (prior == "learned") and "a2c_network.z_prior_mu.weight" in has
    _network(prior).load_state_dict(want)                        # and it loads a reference checkpoint of its own mode, strictly


def test_sphere_prior_beside_a_learned_prior_has_no_effect():
    net = _network("learned", use_vae_sphere_prior=True)
    assert net.use_vae_sphere_prior and not net.sphere_prior and not net.head_modes()["sphere_prior"]
    both = _network("learned", use_vae_fixed_prior=True)
    assert set(both.state_dict()) == set(_network("learned").state_dict())


@pytest.mark.skipif(not refload.available(), reason="needs the reference's network_loader functions")
@pytest.mark.parametrize("prior", PRIORS)
def test_reference_loaders_accept_the_state_dict(prior):
    f = refload.network_loader_functions()
    ck = {"model": _network(prior).state_dict()}
    dec = f["load_z_decoder"](ck, activation="silu", z_type="vae", device="cpu")
    enc = f["load_z_encoder"](ck, activation="silu", z_type="vae", device="cpu")
    assert [m.out_features for m in dec.decoder if isinstance(m, torch.nn.Linear)] == [3096, 2048, 1024, 69]
    assert enc.z_mu.out_features == 32
    assert ("z_prior_mu" in dec) == (prior != "none") and ("z_prior_logvar" in dec) == (prior == "learned")


# ------------------------------------------------------------------------------------------------------------------ rejections, env keys
def test_regulariser_without_a_prior_raises_by_name():
    with pytest.raises(NotImplementedError, match=r"use_vae_prior_regu.*use_vae_prior.*amp_agent\.py:810-813"):
        env_keys.audit(dict(configs.ENV_IM_VAE, use_vae_prior=False, use_vae_prior_regu=True), "test")
    env_keys.audit(dict(configs.ENV_IM_VAE, use_vae_prior=False, use_vae_fixed_prior=True, use_vae_prior_regu=True), "test")


@pytest.mark.parametrize("key", ["z_all", "z_readout"])
def test_unbuilt_latent_options_still_raise_by_name(key):
    with pytest.raises(NotImplementedError, match=key):
        _network("learned", **{key: True})
    with pytest.raises(NotImplementedError, match=key):
        env_keys.audit({key: True}, "test")


def test_other_z_types_and_wide_latents_still_raise():
    with pytest.raises(NotImplementedError, match="z_type"):
        _network("learned", z_type="sphere")
    with pytest.raises(NotImplementedError, match="embedding_size"):
        _network("learned", embedding_size=48)
    for key in ("vae_prior_policy", "distill_z_model"):
        with pytest.raises(NotImplementedError, match=key):
            env_keys.audit({key: True}, "test")


def test_env_keys_classify_the_variants_as_honoured():
    for k in ("use_vae_fixed_prior", "use_vae_sphere_prior", "use_vae_sphere_posterior", "vae_prior_fixed_logvar"):
        assert k in env_keys.HONOURED and k not in env_keys.UNBUILT and k not in env_keys.INERT, k
    for k in ("z_readout", "z_all", "vae_prior_policy", "distill_z_model"):
        assert k in env_keys.UNBUILT, k
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for name in configs.VAE_VARIANTS:
            env_keys.audit(dict(configs.ENV_IM_VAE, **configs.vae_variant_env(name)), name)
