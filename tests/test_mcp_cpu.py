"""CPU: PHC's MCP composer stage (HumanoidImMCP env + amp_mcp network) without a device.

  * the plain-torch twin (tests/mcp_model.py) equals the reference BIT FOR BIT: its ``eval_actor`` against the body of
    AMPMCPBuilder.Network.eval_actor (phc/learning/amp_network_mcp_builder.py:64-86) executed on the twin's own modules, its step composition
    against the statements of HumanoidImMCP.step (phc/env/tasks/humanoid_im_mcp.py:44-71) run on the reference's load_pnn (recorded through
    oracle/refrecord.py, so the tests replay where the reference checkout is absent);
  * the env options of the three shipped MCP env files are classified, the MCP switches are HONOURED, and what is not built raises by name
    before any device is touched;
  * the amp_mcp parameter names, their order and shapes are the twin's (= the reference's creation order).
The GPU half is tests/test_mcp_gpu.py."""
import os
import types
import warnings

import pytest
import torch

from oracle import refload
from oracle.refrecord import RefRecord
from pulse_amd import synthetic as syn
from pulse_amd.env import env_keys as K
from tests import mcp_model as M


def _reference_method(relpath, cls, name, extra=None):
    """A method body of the reference, compiled from its source at run time (for functions outside refload's tables)."""
    ns = refload._namespace()
    ns.update(extra or {})
    src = refload._extract(os.path.join(refload.REFERENCE_ROOT, *relpath), [name], methods_of=cls)[name]
    exec(compile(src, f"<reference:{cls}.{name}>", "exec"), ns)
    return ns[name]


@pytest.mark.parametrize("activation", ["relu", "silu"])
@pytest.mark.parametrize("has_softmax", [False, True])
def test_twin_eval_actor_is_the_reference_eval_actor(request, has_softmax, activation):
    torch.manual_seed(11)
    twin = M.McpTwin(82, [40, 24], 3, activation=activation, has_softmax=has_softmax)
    with torch.no_grad():                                                   # biases are zero-initialised: move them off zero
        for p in twin.parameters():
            if p.dim() == 1 and p.requires_grad:
                p.add_(0.1 * torch.randn_like(p))
    obs = 2 * torch.randn(19, 82, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        mu, sigma = twin.eval_actor(obs)
    assert mu.shape == (19, 3) and sigma.shape == (19, 3) and (sigma == -2.9).all()
    if has_softmax:
        assert torch.allclose(mu.sum(1), torch.ones(19), atol=1e-6)
    else:
        assert (mu >= (0.0 if activation == "relu" else -0.2785)).all()    # the trailing activation's range (min silu = -0.27846)
    want = {}

    def ref(which):
        if not want:
            f = _reference_method(("phc", "learning", "amp_network_mcp_builder.py"), "AMPMCPBuilder.Network", "eval_actor")
            with torch.no_grad():
                want["mu"], want["sigma"] = f(twin.a2c_network, {"obs": obs})
        return want[which]
    with RefRecord(request) as R:
        assert R.equal(mu, R.t("mu", lambda: ref("mu")))
        assert R.equal(sigma, R.t("sigma", lambda: ref("sigma")))


@pytest.mark.parametrize("has_lateral", [False, True])
@pytest.mark.parametrize("activation", ["relu", "silu"])
@pytest.mark.parametrize("discrete_moe", [False, True])
def test_twin_composition_is_the_reference_step(request, discrete_moe, activation, has_lateral):
    ck = syn.synthetic_pnn_checkpoint(3, in_dim=934, units=(96, 64), seed=3, has_lateral=has_lateral)
    g = torch.Generator().manual_seed(1)
    obs = 2 * torch.randn(40, 934, generator=g)
    weights = torch.randn(40, 3, generator=g)
    weights[0], weights[1] = 0.0, -weights[1].abs()                            # a zero row (argmax: the first) and an all-negative row
    got = M.compose(ck, 3, activation, obs, weights, discrete=discrete_moe, has_lateral=has_lateral)
    assert got.shape == (40, 69)
    if discrete_moe:
        x_all = M.pnn_columns(ck["model"], 3, activation, M.normalize_obs(obs, ck["running_mean_std"]["running_mean"],
                                                                            ck["running_mean_std"]["running_var"]), has_lateral)
        assert torch.equal(got, x_all[torch.arange(40), weights.argmax(1)] + 0.0)

    def want():
        step = _reference_method(("phc", "env", "tasks", "humanoid_im_mcp.py"), "HumanoidImMCP", "step")
        pnn = refload.pnn_reference()["load_pnn"](ck, num_prim=3, has_lateral=has_lateral, activation=activation, device="cpu")
        seen = {}
        stub = types.SimpleNamespace(obs_buf=obs.clone(), running_mean=ck["running_mean_std"]["running_mean"],
                                     running_var=ck["running_mean_std"]["running_var"], discrete_mcp=discrete_moe, num_prim=3, has_pnn=True, pnn=pnn,
                                     pre_physics_step=lambda a: seen.setdefault("actions", a), _physics_step=lambda: None,
                                     post_physics_step=lambda: None, device="cuda:0", dr_randomizations={})
        step(stub, weights.clone())
        return seen["actions"]
    with RefRecord(request) as R:
        assert R.equal(got, R.t("actions", want))


MCP_ENV_FILES = ["phc_kp_mcp_iccv.yaml", "phc_shape_mcp_iccv.yaml", "env_im_getup_mcp.yaml"]


def _mcp_env_configs():
    import yaml
    out = {}
    for f in MCP_ENV_FILES:
        with open(os.path.join(refload.REFERENCE_ROOT, "phc", "data", "cfg", "env", f)) as fh:
            d = yaml.safe_load(fh)
        out[f] = d["env"] if isinstance(d.get("env"), dict) else d
    return out


def test_shipped_mcp_env_files_pass_the_audit_with_every_mcp_key_classified(request):
    with RefRecord(request) as R:
        configs = R.obj("env_configs", _mcp_env_configs)
    assert sorted(configs) == sorted(MCP_ENV_FILES)
    for name, env in configs.items():
        assert env.get("has_pnn") is True and "num_prim" in env, name
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                     # (legacy spellings the reference does not read either)
            K.audit(env, name)
        for k in ("has_pnn", "num_prim", "has_lateral"):
            assert k in env and k in K.HONOURED, (name, k)
    for k in ("has_pnn", "discrete_moe", "z_activation", "num_prim", "has_lateral"):
        assert k in K.HONOURED and k not in K.INERT and k not in K.UNBUILT, k
    for k in ("training_prim", "actors_to_load"):                               # steer PNN training, which is not built
        assert k in K.INERT, k


def test_mcp_switches_do_not_warn_as_unknown():
    for k in ("has_pnn", "discrete_moe", "z_activation"):
        K._warned.discard(k)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        K.audit({"has_pnn": True, "discrete_moe": False, "z_activation": "relu", "num_prim": 4, "has_lateral": False}, "test")


@pytest.mark.parametrize("cls", ["HumanoidImMCP", "HumanoidImMCPGetup"])
def test_unbuilt_mcp_options_raise_by_name_without_a_device(cls):
    from pulse_amd.env import humanoid_im_mcp as H
    C = getattr(H, cls)
    with pytest.raises(NotImplementedError, match="has_pnn"):
        C({"env": {"has_pnn": False, "num_prim": 4}}, None, None)
    with pytest.raises(NotImplementedError, match="has_pnn"):                   # the reference's default is False (:18)
        C({"env": {"num_prim": 4}}, None, None)
    for ht in ("smplx", "smplh"):
        with pytest.raises(NotImplementedError, match=f"{ht}.*{cls}"):
            C({"env": {"has_pnn": True, "num_prim": 4}, "robot": {"humanoid_type": ht, "has_upright_start": False}}, None, None)
    with pytest.raises(NotImplementedError, match="num_prim"):
        C({"env": {"has_pnn": True, "num_prim": 33}}, None, None)
    with pytest.raises(NotImplementedError, match="z_activation"):
        C({"env": {"has_pnn": True, "z_activation": "gelu"}}, None, None)


def test_amp_mcp_parameter_names_order_and_shapes_are_the_twins():
    from pulse_amd.learning.network_mcp import mcp_parameter_layout
    twin = M.McpTwin(82, [40, 24], 3)
    want = twin.layout()
    assert [k for k, _ in want][:4] == ["a2c_network.actor_mlp.0.weight", "a2c_network.actor_mlp.0.bias", "a2c_network.actor_mlp.2.weight",
                                        "a2c_network.actor_mlp.2.bias"]
    assert [k for k, _ in want][-6:] == [f"a2c_network.composer.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
    assert mcp_parameter_layout([40, 24], 3, 82) == want
    assert "a2c_network.sigma" in twin.state_dict()                            # the fixed sigma travels with the checkpoint


def test_mcp_configs_resolve_without_a_device():
    from pulse_amd import configs
    cfg, n = configs.agent_config("mcp_small")
    assert n == 64 and cfg["horizon_length"] == 16 and cfg["minibatch_size"] == 256 and cfg["_agent_kind"] == "amp" and cfg["_env_kind"] == "mcp"
    assert cfg["network"]["name"] == "amp_mcp" and cfg["network"]["has_softmax"] is False
    cfg, n = configs.agent_config("mcp")
    assert cfg["network"]["mlp"] == {"units": [1024, 512], "activation": "relu", "d2rl": False, "initializer": {"name": "default"}}
    assert (cfg["horizon_length"], cfg["minibatch_size"], cfg["learning_rate"], cfg["mini_epochs"]) == (32, 16384, 2e-5, 6)
    assert configs.ENV_MCP["num_prim"] == 4 and configs.ENV_MCP["has_pnn"] and configs.ENV_MCP["obs_v"] == 7
    ck = syn.synthetic_pnn_checkpoint(4, in_dim=50, units=(12, 8), seed=2, has_lateral=True)
    ck2 = syn.synthetic_pnn_checkpoint(4, in_dim=50, units=(12, 8), seed=2, has_lateral=True)
    assert all(torch.equal(v, ck2["model"][k]) for k, v in ck["model"].items())
    assert "a2c_network.pnn.u.2.2.0.weight" in ck["model"] and ck["model"]["a2c_network.mu.bias"].shape == (69,)
    assert set(ck["running_mean_std"]) >= {"running_mean", "running_var"} and ck["running_mean_std"]["running_mean"].shape == (50,)


FIX = os.path.join(os.path.dirname(__file__), "golden", "ckpt_mcp_small.pt")


def test_reference_composer_loader_reads_our_checkpoint_and_reproduces_mu(request):
    """A checkpoint the MI355X agent wrote after two epochs of ``mcp_small`` (tools/make_mcp_ckpt_fixture.py, has_softmax: False): its composer
    loads into the reference's load_mcp_mlp(..., mlp_name="composer") (phc/learning/network_loader.py:11-52, trailing activation included) and
    gives the mu the HIP path computed from the same observations, within test_teacher.py's figure for these MLPs (2e-5)."""
    from pulse_amd.learning.network_mcp import mcp_parameter_layout
    R = RefRecord(request)
    ck = torch.load(FIX, map_location="cpu", weights_only=False)
    fx = ck["fixture"]
    units, act = fx["network"]["mlp"]["units"], fx["network"]["mlp"]["activation"]
    assert fx["network"]["has_softmax"] is False
    obs = fx["obs_buf"]
    layout = [(k, tuple(s)) for k, s in ck["model_layout"] if k != "a2c_network.sigma"]
    assert layout == mcp_parameter_layout(units, 4, obs.shape[1])                # the whole checkpoint: reference names, reference order
    assert ("a2c_network.sigma", (4,)) in [(k, tuple(s)) for k, s in ck["model_layout"]]
    rms = ck["running_mean_std"]
    x = torch.clamp((obs - rms["running_mean"].float()) / torch.sqrt(rms["running_var"].float() + 1e-05), min=-5.0, max=5.0)
    if R.live:
        composer = refload.pnn_reference()["load_mcp_mlp"](ck, activation=act, device="cpu", mlp_name="composer")
    assert R.obj("widths", lambda: [m.out_features for m in composer if isinstance(m, torch.nn.Linear)]) == units + [4]
    assert R.obj("trailing", lambda: type(composer[-1]).__name__) == {"relu": "ReLU", "silu": "SiLU"}[act]
    want = R.t("mu", lambda: composer(x))
    assert fx["mu"].shape == want.shape == (obs.shape[0], 4) and fx["mu"].abs().max() > 0
    import numpy as np
    np.testing.assert_allclose(fx["mu"].numpy(), want.numpy(), atol=2e-5, rtol=2e-5)
    R.close()
