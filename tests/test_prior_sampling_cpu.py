"""CPU: generation from the PULSE prior (z drawn from the prior, the encoder skipped).

  * tests/prior_sampling_model.py (the plain-torch restatement the GPU tests compare against) equals tests/golden/prior_sampling.npz --
    outputs of the reference's own form_embedding under flags.debug -- bit for bit, for every prior x posterior the reference can run;
  * where the reference checkout is present, a fresh generate() reproduces the committed fixture key by key;
  * the generator's conditions (the fixture cannot hide a failure) hold on the committed file;
  * the new entry point's struct as the C compiler lays it out, the ABI version, the argument errors that need no device;
  * the model / player options are validated without a device.

The prior-mean and constant-log-variance variants are commented out in the reference (amp_network_z_builder.py:109-111): no statement of
it runs them, so the restatement is their yardstick; here they are only held to their defining identities."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden_prior_sampling as GP  # noqa: E402
import prior_sampling_model as PM  # noqa: E402
from oracle import refload  # noqa: E402
from pulse_amd import _lib, configs  # noqa: E402
from pulse_amd import kernels as K  # noqa: E402
from pulse_amd.learning import network_z, players  # noqa: E402

CASES = [(p, s) for p in GP.PRIORS for s in GP.POSTS]


@pytest.fixture(scope="module")
def fx():
    return GP.load()


@pytest.fixture(scope="module")
def d():
    return GP.inputs()


def same(t, a):
    return np.array_equal(t.detach().numpy(), a)


def test_inputs_are_the_ones_the_fixture_was_made_from(fx, d):
    for k, v in GP.input_sums(d).items():
        assert float(v) == float(fx[k]), k


@pytest.mark.parametrize("prior,post", CASES)
def test_restatement_equals_reference_outputs(fx, d, prior, post):
    net = GP.make_net(prior, post).train()
    eps = torch.from_numpy(fx["eps"])
    with torch.no_grad():
        assert same(PM.prior_z(net, d["obs"], eps), fx[f"z/{prior}/{post}"])
        mu, lv = PM.raw_prior_heads(net, d["obs"])
        if prior == "none":
            assert mu is None and same(eps if post == "gauss" else PM.project_to_norm(eps, GP.GV.NORM), fx[f"z/none/{post}"])
            return
        assert same(mu, fx[f"heads/{prior}/mu"]) and (prior != "learned" or same(lv, fx["heads/learned/logvar"]))
        # from the stored heads alone (what the GPU test feeds the kernel)
        heads_mu = torch.from_numpy(fx[f"heads/{prior}/mu"])
        heads_lv = torch.from_numpy(fx["heads/learned/logvar"]) if prior == "learned" else None
        assert same(PM.z_from_prior_heads(heads_mu, heads_lv, eps, **PM.net_modes(net)), fx[f"z/{prior}/{post}"])
        pm, pv = net.compute_prior(d["obs"])
        assert same(pm, fx[f"prior/{prior}/{post}/mu"]) and same(pv, fx[f"prior/{prior}/{post}/logvar"])


@pytest.mark.parametrize("prior,post", [c for c in CASES if c[0] != "none"])
def test_commented_variants_defining_identities(fx, d, prior, post):
    """z = prior_mu (:109) and reparameterize(prior_mu, const) (:110-111), written out against compute_prior's own outputs."""
    net = GP.make_net(prior, post)
    eps = torch.from_numpy(fx["eps"])
    pm = torch.from_numpy(fx[f"prior/{prior}/{post}/mu"])
    proj = (lambda z: PM.project_to_norm(z, GP.GV.NORM)) if GP.GV.POSTS[post] else (lambda z: z)
    with torch.no_grad():
        assert torch.equal(PM.prior_z(net, d["obs"], None), proj(pm))
        for c in (-2.3, -1.5):
            want = proj(pm + eps * torch.exp(0.5 * (torch.ones_like(pm) * c)))
            assert torch.equal(PM.prior_z(net, d["obs"], eps, logvar_override=c), want)
        assert not torch.equal(PM.prior_z(net, d["obs"], eps, logvar_override=-2.3), PM.prior_z(net, d["obs"], eps))


def test_generator_conditions_hold_on_the_committed_fixture(fx):
    GP.check_conditions(fx)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "prior_sampling.npz")) <= GP.MAX_BYTES
    assert fx["eps"].shape == fx["z/learned/gauss"].shape == (GP.GV.HORIZON * GP.GV.NSEQ, GP.GV.SIZES["embedding_size"])


@pytest.mark.skipif(not refload.available(), reason="reference checkout not present: the fixture stands in for it")
def test_reference_method_body_reproduces_the_fixture(fx):
    live = GP.generate()
    assert set(live) == set(fx)
    for k in sorted(fx):
        assert np.array_equal(live[k], fx[k]), k
    flags = GP.GV.reference_flags()
    assert flags.debug is False and flags.test is False              # the generator leaves the reference's switches as it found them


# ------------------------------------------------------------------------------------------------------------------ the entry point
def test_entry_point_binding():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.VaeEmbedPriorArgs) == lib.pulse_sizeof_vae_embed_prior_args()
    assert lib.pulse_abi_version() == 36                            # an added entry point: no existing struct or signature changed
    assert ctypes.sizeof(_lib.VaeEmbedArgs) == lib.pulse_sizeof_vae_embed_args()
    assert lib.pulse_vae_embed_prior(None, None) == -1 and b"null args" in lib.pulse_last_error()
    a = _lib.VaeEmbedPriorArgs()
    assert lib.pulse_vae_embed_prior(ctypes.byref(a), None) == 0      # zero rows: nothing to do
    a.rows, a.embedding_size = 4, 33
    assert lib.pulse_vae_embed_prior(ctypes.byref(a), None) == -1 and b"embedding_size <= 32" in lib.pulse_last_error()
    a.embedding_size, a.prior_mode = 32, 3
    assert lib.pulse_vae_embed_prior(ctypes.byref(a), None) == -1 and b"prior_mode" in lib.pulse_last_error()
    header = open(os.path.join(ROOT, "include", "pulse_hip.h")).read()
    assert "amp_network_z_builder.py:101-119, 226-248" in header
    assert (K.PRIOR_LEARNED, K.PRIOR_FIXED, K.PRIOR_NONE) == (0, 1, 2)


# ------------------------------------------------------------------------------------------------------------------ options, no device
def test_check_z_source_by_prior_mode():
    for src in network_z.Z_SOURCES:
        network_z.check_z_source(src, None, None)
    network_z.check_z_source("posterior", None, K.PRIOR_NONE)
    network_z.check_z_source("normal", None, K.PRIOR_NONE)
    for mode in (K.PRIOR_LEARNED, K.PRIOR_FIXED):
        network_z.check_z_source("prior", -2.3, mode)
        network_z.check_z_source("prior_mean", None, mode)
        with pytest.raises(ValueError, match="without a prior"):
            network_z.check_z_source("normal", None, mode)
    for src in ("prior", "prior_mean"):
        with pytest.raises(ValueError, match=r"use_vae_prior.*use_vae_fixed_prior"):
            network_z.check_z_source(src, None, K.PRIOR_NONE)
    with pytest.raises(ValueError, match="z_source 'encoder'"):
        network_z.check_z_source("encoder", None, K.PRIOR_LEARNED)
    for bad in ("cold", True, float("nan")):
        with pytest.raises(ValueError, match="prior_logvar"):
            network_z.check_z_source("prior", bad, K.PRIOR_LEARNED)
    with pytest.raises(ValueError, match="prior_logvar"):
        network_z.check_z_source("prior_mean", -2.3, K.PRIOR_LEARNED)
    assert network_z.prior_mode_of({}) == K.PRIOR_LEARNED and network_z.prior_mode_of({"use_vae_prior": False}) == K.PRIOR_NONE
    assert network_z.prior_mode_of({"use_vae_prior": True, "use_vae_fixed_prior": True}) == K.PRIOR_LEARNED
    assert network_z.prior_mode_of({"use_vae_prior": False, "use_vae_fixed_prior": True}) == K.PRIOR_FIXED


def _stub_env(detail):
    def boom(*a, **k):
        raise AssertionError("the env was touched before the options were validated")
    task = types.SimpleNamespace(get_task_obs_size_detail=lambda: detail)
    return types.SimpleNamespace(env=types.SimpleNamespace(task=task), get_env_info=boom, num_envs=4)


@pytest.mark.parametrize("cls", [players.CommonPlayer, players.AMPPlayerContinuous])
def test_player_validates_its_options_before_any_device_work(cls):
    """No GPU here: a player that got as far as building its agent would fail otherwise (or reach the stub env's get_env_info)."""
    learned, none = {"use_vae_prior": True}, {"use_vae_prior": False}
    base = {"network": {"name": "amp_z"}, "device": "cuda:0"}
    with pytest.raises(ValueError, match="z_source 'sideways'"):
        cls(dict(base, player={"z_source": "sideways"}, vec_env=_stub_env(learned)))
    with pytest.raises(ValueError, match=r"use_vae_prior.*use_vae_fixed_prior"):
        cls(dict(base, player={"z_source": "prior"}, vec_env=_stub_env(none)))
    with pytest.raises(ValueError, match="'normal'.*without a prior"):
        cls(dict(base, player={"z_source": "normal"}, vec_env=_stub_env(learned)))
    with pytest.raises(ValueError, match="network 'amp'"):
        cls(dict(base, network={"name": "amp"}, player={"z_source": "prior"}, vec_env=_stub_env({})))
    with pytest.raises(ValueError, match="prior_logvar"):
        cls(dict(base, player={"z_source": "prior", "prior_logvar": "warm"}, vec_env=_stub_env(learned)))
    assert players.check_z_source_options(dict(base, player={"z_source": "prior", "prior_logvar": -1.5}, vec_env=_stub_env(learned))) == ("prior", -1.5)
    assert players.check_z_source_options(base) == ("posterior", None)
    assert players.check_z_source_options(dict(base, network={"name": "amp"})) == ("posterior", None)      # the default asks nothing of the network


def test_make_player_validates_against_the_config_before_the_env_exists(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("make_env ran before the options were validated")
    monkeypatch.setattr(configs, "make_env", boom)
    with pytest.raises(ValueError, match="z_source 'sideways'"):
        configs.make_player("cfg3_small", z_source="sideways")
    with pytest.raises(ValueError, match=r"use_vae_prior.*use_vae_fixed_prior"):
        configs.make_player("cfg3_small", z_source="prior", env_overrides=configs.vae_variant_env("none"))
    with pytest.raises(ValueError, match="'normal'.*without a prior"):
        configs.make_player("cfg3_small", z_source="normal")
    with pytest.raises(ValueError, match="'normal'.*without a prior"):
        configs.make_player("cfg3_small", z_source="normal", env_overrides=configs.vae_variant_env("fixed"))
    for name, net in (("cfg1", "amp"), ("pnn_small", "amp_pnn"), ("speed_z_small", "amp_z_reader")):
        with pytest.raises(ValueError, match=f"network '{net}'"):
            configs.make_player(name, z_source="prior")
    for ok in (dict(z_source="prior"), dict(z_source="prior", prior_logvar=-2.3), dict(z_source="prior_mean"),
               dict(z_source="normal", env_overrides=configs.vae_variant_env("none")),
               dict(z_source="prior", env_overrides=configs.vae_variant_env("fixed_sphere_post"))):
        with pytest.raises(AssertionError, match="make_env ran"):          # valid options: construction goes on to the env
            configs.make_player("cfg3_small", **ok)
