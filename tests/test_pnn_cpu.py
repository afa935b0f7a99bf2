"""CPU: PHC's primitive stage (``network: amp_pnn``) without a device.

  * the plain-torch twin (tests/pnn_model.py) equals the reference BIT FOR BIT: its PNN against the reference's own class (parameter names, order,
    shapes, ``requires_grad`` after ``freeze_pnn``, ``forward``), its ``eval_actor`` against the body of AMPPNNBuilder.Network.eval_actor
    (phc/learning/amp_network_pnn_builder.py:62-89) run on the reference's PNN (recorded through oracle/refrecord.py, so the tests replay where
    the reference checkout is absent);
  * ``pnn_parameter_layout`` is the twin's parameter list; both network classes hand out and take back a checkpoint under those names on the CPU;
  * the reference's ``load_pnn`` reads that checkpoint and reproduces the twin's columns;
  * what is not built raises by name before a device is touched; the four env keys default to the reference's; the runner knows the name.
The GPU half is tests/test_pnn_gpu.py."""
import os
import types

import pytest
import torch

from oracle import refload
from oracle.refrecord import RefRecord
from pulse_amd import configs
from pulse_amd.learning import network_pnn as NP
from tests import pnn_model as M

OBS, UNITS, A, P, ROWS = 50, [36, 32], 7, 3, 7


def _reference_method(relpath, cls, name, extra=None):
    """A method body of the reference, compiled from its source at run time (as tests/test_mcp_cpu.py does)."""
    ns = refload._namespace()
    ns.update(extra or {})
    src = refload._extract(os.path.join(refload.REFERENCE_ROOT, *relpath), [name], methods_of=cls)[name]
    exec(compile(src, f"<reference:{cls}.{name}>", "exec"), ns)
    return ns[name]


def _params(units=UNITS, activation="relu"):
    return dict(configs.NETWORK_PNN, mlp=dict(configs.NETWORK_PNN["mlp"], units=list(units), activation=activation))


def _detail(training_prim, has_lateral, num_prim=P):
    return {"num_prim": num_prim, "training_prim": training_prim, "actors_to_load": 0, "has_lateral": has_lateral}


def _twin(training_prim, has_lateral, activation="relu", seed=21):
    torch.manual_seed(seed)
    return M.PnnTwin(OBS, UNITS, A, P, training_prim, has_lateral=has_lateral, activation=activation).jitter_biases()


def _reference_pnn(twin, has_lateral, activation, training_prim):
    """The reference's PNN class with the twin's weights, frozen at ``training_prim``."""
    ref = refload.pnn_reference()["PNN"]({"input_size": OBS, "units": list(UNITS), "activation": activation, "dense_func": torch.nn.Linear},
                                         output_size=A, numCols=P, has_lateral=has_lateral)
    ref.load_state_dict(twin.a2c_network.pnn.state_dict(), strict=True)
    ref.freeze_pnn(training_prim)
    return ref


@pytest.mark.parametrize("activation", ["relu", "silu"])
@pytest.mark.parametrize("has_lateral", [False, True])
@pytest.mark.parametrize("training_prim", [0, 1, 2])
def test_twin_is_the_reference_pnn_and_eval_actor(request, training_prim, has_lateral, activation):
    twin = _twin(training_prim, has_lateral, activation)
    obs = 2 * torch.randn(ROWS, OBS, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        mu, sigma = twin.eval_actor(obs)
        cols = twin.columns(obs)
    assert mu.shape == (ROWS, A) and sigma.shape == (ROWS, A) and (sigma == -2.9).all() and cols.shape == (ROWS, P, A)
    if not has_lateral or training_prim == P - 1:
        assert torch.equal(cols[:, training_prim], mu)
    mine = [[k, list(p.shape), bool(p.requires_grad)] for k, p in twin.a2c_network.pnn.named_parameters()]
    # freeze_pnn (:41-46): actors[:idx]; u[:idx - 1] -- for idx 0 the slice ends at -1 (every lateral row but the last), for idx 1 it is empty
    frozen_u = {0: [0], 1: [], 2: [0]}[training_prim]
    for k, _, rg in mine:
        if k.startswith("actors."):
            assert rg == (int(k.split(".")[1]) >= training_prim), k
        else:
            assert rg == (int(k.split(".")[1]) not in frozen_u), k
    want = {}

    def ref(which):
        if not want:
            pnn = _reference_pnn(twin, has_lateral, activation, training_prim)
            want["params"] = [[k, list(p.shape), bool(p.requires_grad)] for k, p in pnn.named_parameters()]
            f = _reference_method(("phc", "learning", "amp_network_pnn_builder.py"), "AMPPNNBuilder.Network", "eval_actor")
            net = twin.a2c_network
            stub = types.SimpleNamespace(actor_cnn=net.actor_cnn, pnn=pnn, training_prim=training_prim, is_discrete=False, is_multi_discrete=False,
                                         is_continuous=True, space_config={"fixed_sigma": True}, sigma_act=net.sigma_act, sigma=net.sigma)
            with torch.no_grad():
                want["mu"], want["sigma"] = f(stub, {"obs": obs})
                want["cols"] = torch.stack(list(pnn(obs, idx=-1)[1]), dim=1)
        return want[which]
    with RefRecord(request) as R:
        assert mine == R.obj("params", lambda: ref("params"))
        assert R.equal(mu, R.t("mu", lambda: ref("mu")))
        assert R.equal(sigma, R.t("sigma", lambda: ref("sigma")))
        assert R.equal(cols, R.t("cols", lambda: ref("cols")))


@pytest.mark.parametrize("has_lateral", [False, True])
def test_parameter_layout_is_the_twins(has_lateral):
    twin = M.PnnTwin(OBS, UNITS, A, P, 1, has_lateral=has_lateral)
    want = twin.layout()
    assert not any(".actor_mlp." in k for k, _ in want)                          # deleted (:52)
    assert [k for k, _ in want][:8] == [f"a2c_network.critic_mlp.{i}.{p}" for i in (0, 2) for p in ("weight", "bias")] + \
        ["a2c_network.value.weight", "a2c_network.value.bias", "a2c_network.mu.weight", "a2c_network.mu.bias"]
    assert want[8][0] == "a2c_network.pnn.actors.0.0.weight"
    assert NP.pnn_parameter_layout(UNITS, P, OBS, A, has_lateral) == want
    assert ("a2c_network.pnn.u.1.1.1.weight", (A, UNITS[1])) in want if has_lateral else not any(".pnn.u." in k for k, _ in want)


def _network(training_prim, has_lateral, activation="relu"):
    if has_lateral and training_prim > 0:
        return NP.AMPPNNLateralNetwork(_params(activation=activation), actions_num=A, self_obs_size=20, task_obs_size=OBS - 20,
                                       task_obs_size_detail=_detail(training_prim, True), device="cpu")
    return NP.AMPPNNNetwork(_params(activation=activation), actions_num=A, input_shape=(OBS,), task_obs_size_detail=_detail(training_prim, has_lateral),
                            device="cpu")


@pytest.mark.parametrize("has_lateral", [False, True])
@pytest.mark.parametrize("training_prim", [0, 1, 2])
def test_state_dict_speaks_the_twins_names_and_a_shared_seed_reproduces_it(training_prim, has_lateral):
    torch.manual_seed(33)
    twin = M.PnnTwin(OBS, UNITS, A, P, training_prim, has_lateral=has_lateral)
    torch.manual_seed(33)
    net = _network(training_prim, has_lateral)
    sd, ref = net.state_dict(), twin.state_dict_ref()
    # names and creation order (torch lists a module's own parameter, sigma, in front of its children; the checkpoint keeps it behind mu)
    assert [k for k in sd if k != "a2c_network.sigma"] == [k for k in ref if k != "a2c_network.sigma"]
    assert list(sd).index("a2c_network.sigma") == list(sd).index("a2c_network.mu.bias") + 1 and set(sd) == set(ref)
    for k, v in ref.items():
        assert torch.equal(sd[k], v), k                                         # same draws in the same order, biases zeroed
    # and a checkpoint goes in and comes out bit for bit, whichever column the flat buffer holds
    other = _twin(training_prim, has_lateral, seed=4).state_dict_ref()
    net.load_state_dict(other)
    back = net.state_dict()
    assert all(torch.equal(back[k], v) for k, v in other.items())
    with pytest.raises(KeyError):
        net.load_state_dict({k: v for k, v in other.items() if k != "a2c_network.pnn.actors.2.4.bias"})
    if not (has_lateral and training_prim > 0):
        # the trained column and the critic are the flat buffer's; everything else is carried outside it
        inside = set(net._flat_names())
        assert inside == {k for k in ref if ".critic_mlp." in k or ".value." in k or f".pnn.actors.{training_prim}." in k}
        assert set(net.carried) == set(ref) - inside - {"a2c_network.sigma"}
        plain_count = sum(v.numel() for k, v in ref.items() if k in inside)
        assert net.parameters_count() >= plain_count and set(net.named_gradients()) == inside


@pytest.mark.parametrize("has_lateral", [False, True])
def test_reference_load_pnn_reads_our_checkpoint(request, has_lateral):
    twin = _twin(2, has_lateral, "silu", seed=8)
    net = _network(2, has_lateral, "silu")
    net.load_state_dict(twin.state_dict_ref())
    ck = {"model": net.state_dict()}
    obs = 2 * torch.randn(ROWS, OBS, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        cols = twin.columns(obs)

    def want():
        pnn = refload.pnn_reference()["load_pnn"](ck, num_prim=P, has_lateral=has_lateral, activation="silu", device="cpu")
        assert not any(p.requires_grad for p in pnn.actors.parameters())
        with torch.no_grad():
            return torch.stack(list(pnn(obs, idx=-1)[1]), dim=1)
    with RefRecord(request) as R:
        assert R.equal(cols, R.t("cols", want))


def test_rejections_by_name_without_a_device():
    chk = lambda d, units=UNITS, **kw: NP.check_pnn_options(_params(units), d, A, **kw)
    for tp in (-1, 3):
        with pytest.raises(ValueError, match="training_prim"):
            chk(_detail(tp, False))
    with pytest.raises(NotImplementedError, match="num_prim"):
        chk(_detail(0, False, num_prim=33))
    with pytest.raises(NotImplementedError, match="num_prim"):
        chk(_detail(0, False, num_prim=0))
    with pytest.raises(NotImplementedError, match=r"pnn\.py:98"):
        chk(_detail(1, True), units=[36, 32, 16])
    with pytest.raises(NotImplementedError, match="mixed_precision.*has_lateral|has_lateral.*mixed_precision"):
        chk(_detail(1, True), mixed_precision=True)
    with pytest.raises(ValueError, match="actions_num"):
        chk(_detail(1, False), env_actions=69)
    assert chk(_detail(0, True), mixed_precision=True) == (3, 0, True, False)   # column 0 with laterals is the plain column (pnn.py:88-90)
    assert chk(_detail(2, True)) == (3, 2, True, True)
    assert chk(_detail(1, False, num_prim=32), units=[8, 8, 8], mixed_precision=True, env_actions=A) == (32, 1, False, False)
    # the constructors go through the same check
    with pytest.raises(ValueError, match="training_prim"):
        NP.AMPPNNNetwork(_params(), actions_num=A, input_shape=(OBS,), task_obs_size_detail=_detail(3, False), device="cpu")
    task = types.SimpleNamespace(cfg={"env": {"num_prim": 3, "training_prim": 2, "has_lateral": True}}, num_actions=A,
                                 get_task_obs_size_detail=lambda: {})
    with pytest.raises(NotImplementedError, match="mixed_precision"):
        NP.build_pnn_model(_params(), task=task, actions_num=A, input_shape=(OBS,), device="cuda:0", mixed_precision=True)


def test_the_four_keys_default_to_the_references(request):
    def ref_defaults():
        import re
        with open(os.path.join(refload.REFERENCE_ROOT, "phc", "env", "tasks", "humanoid_im.py")) as f:
            src = f.read()
        found = dict(re.findall(r"task_obs_detail\['(num_prim|training_prim|actors_to_load|has_lateral)'\] = self\.cfg\['env'\]\.get\(\"\w+\", (\w+)\)", src))
        return {k: (v == "True" if v in ("True", "False") else int(v)) for k, v in found.items()}
    with RefRecord(request) as R:
        want = R.obj("defaults", ref_defaults)
    assert want == {"num_prim": 2, "training_prim": 1, "actors_to_load": 2, "has_lateral": True}
    assert NP.pnn_options({}) == want == NP.PNN_DEFAULTS
    got = NP.pnn_options({"num_prim": 4, "has_lateral": False}, {"obs_v": 6})
    assert got == {"obs_v": 6, "num_prim": 4, "training_prim": 1, "actors_to_load": 2, "has_lateral": False}
    from pulse_amd.env import env_keys
    for k in ("training_prim", "actors_to_load"):
        assert k in env_keys.INERT and "amp_pnn" in env_keys.INERT[k]
    for name in ("pnn", "pnn_small", "pnn_lateral_small"):                      # the configs' own cfg["env"] passes the audit
        env_keys.audit(dict(configs.ENV_IM, **configs.agent_config(name)[0]["_env_overrides"]), name)


def test_runner_and_configs_know_amp_pnn():
    from pulse_amd import runner as Rn
    r = Rn.build_alg_runner()
    r.model_builder.network_factory.create("amp_pnn")                            # registered (run_hydra.py:261)
    cfg, n = configs.agent_config("pnn")
    c5, n5 = configs.agent_config("cfg5")
    assert n == n5 == 8192 and cfg["network"]["name"] == "amp_pnn" and cfg["mixed_precision"] is True and cfg["_env_kind"] == c5["_env_kind"] == "amp"
    assert {k: v for k, v in cfg["network"].items() if k not in ("name", "discrete")} == {k: v for k, v in c5["network"].items() if k != "name"}
    assert {k: v for k, v in cfg.items() if k not in ("network", "_env_overrides")} == {k: v for k, v in c5.items() if k not in ("network", "_env_overrides")}
    assert cfg["_env_overrides"] == {"num_prim": 4, "training_prim": 0, "actors_to_load": 0, "has_lateral": False}
    cfg, n = configs.agent_config("pnn_small")
    assert n == 64 and cfg["network"]["mlp"]["units"] == [512, 512] and not cfg["mixed_precision"]
    cfg, n = configs.agent_config("pnn_lateral_small")
    assert n == 64 and cfg["network"]["mlp"]["units"] == [36, 32] and not cfg["mixed_precision"]
    assert cfg["_env_overrides"] == {"num_prim": 3, "training_prim": 2, "actors_to_load": 2, "has_lateral": True}
