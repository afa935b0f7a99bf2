"""GPU: PHC's primitive stage (``network: amp_pnn``) on the HIP path.

  * without laterals the network IS A2CNetwork with another checkpoint surface: mu, value and every gradient are BIT-IDENTICAL to a plain ``amp``
    network holding the trained column and the critic (the same launches), fp32 and ``mixed_precision``; the columns that do not train and
    ``a2c_network.mu.*`` keep their bits through forward, backward and an Adam step;
  * with laterals the graph network against the plain-torch twin's autograd (tests/pnn_model.py, itself held to the reference bit for bit by
    tests/test_pnn_cpu.py), at the bounds tests/test_mcp_gpu.py holds ``amp_mcp`` to against its twin (forward 5e-5, gradients 3e-4 of the
    largest magnitude: the same GEMM plans); frozen and unevaluated parameters get exactly zero;
  * the agents end to end, moving on to the next primitive, the consumers of the checkpoint (PnnTeacher, HumanoidImMCP), the runner, and the
    launch audit of tests/test_gemm_launch_audit_gpu.py over the new configs.
"""
import numpy as np
import pytest
import torch

from pulse_amd import configs, kernels as K
from pulse_amd.learning import network_pnn as NP
from pulse_amd.learning.network import A2CNetwork
from tests import mcp_model as MM
from tests import pnn_model as M
from tests.test_gemm_launch_audit_gpu import auditor  # noqa: F401  (the fixture that wraps the GEMM descriptor builders and launchers)

pytestmark = pytest.mark.gpu

OBS, A, P, ROWS = 50, 7, 3, 130


def _params(units, activation="relu", name="amp_pnn"):
    return dict(configs.NETWORK_PNN, name=name, mlp=dict(configs.NETWORK_PNN["mlp"], units=list(units), activation=activation))


def _detail(training_prim, has_lateral, num_prim=P):
    return {"num_prim": num_prim, "training_prim": training_prim, "actors_to_load": 0, "has_lateral": has_lateral}


def _pass(net, obs, dmu, dval):
    """One training forward + backward over ``obs`` with the given d loss / d (mu, value): (mu, value) clones; the gradient is in net.grad."""
    m = obs.shape[0]
    ws = net.workspace(m, train=True)
    ws["x"].zero_()
    ws["x"][:, :obs.shape[1]] = obs
    net.train()
    net.forward(ws, m)
    mu, val = ws["mu"].clone(), ws["val"].clone()
    ws["dmu"].copy_(dmu)
    ws["dval"].copy_(dval)
    if ws.get("b16"):
        raise AssertionError("this shape was chosen to stay on the fp32-storage plans")
    net.backward(ws, m)
    return mu, val


# --------------------------------------------------------------------------------------------------------------------- 1. no laterals
@pytest.mark.parametrize("mixed_precision", [False, True])
def test_plain_column_is_the_amp_network_bit_for_bit(dev, mixed_precision):
    units, t = [64, 32], 1
    torch.manual_seed(3)
    twin = M.PnnTwin(OBS, units, A, P, t).jitter_biases()
    net = NP.AMPPNNNetwork(_params(units), actions_num=A, input_shape=(OBS,), task_obs_size_detail=_detail(t, False), device=dev)
    net.load_state_dict(twin.state_dict_ref())
    plain = A2CNetwork(_params(units, name="amp"), actions_num=A, input_shape=(OBS,), device=dev)
    sd = net.state_dict()
    col = {f"a2c_network.actor_mlp.{i}.{p}": sd[f"a2c_network.pnn.actors.{t}.{i}.{p}"] for i in (0, 2) for p in ("weight", "bias")}
    col.update({f"a2c_network.mu.{p}": sd[f"a2c_network.pnn.actors.{t}.4.{p}"] for p in ("weight", "bias")})
    plain.load_state_dict({**{k: v for k, v in sd.items() if ".critic_mlp." in k or ".value." in k or k.endswith(".sigma")}, **col})
    assert net.n_flat == plain.n_flat and torch.equal(net.flat, plain.flat)       # the same flat buffer: column t in the actor slots
    net.mixed_precision = plain.mixed_precision = mixed_precision
    g = torch.Generator().manual_seed(9)
    obs = torch.randn(ROWS, OBS, generator=g).clamp(-5, 5).to(dev)
    dmu, dval = torch.randn(ROWS, A, generator=g).to(dev), torch.randn(ROWS, 1, generator=g).to(dev)
    carried = {k: v.clone() for k, v in net.carried.items()}
    assert set(carried) == {k for k in sd if (".pnn.actors." in k and f".actors.{t}." not in k) or ".mu." in k}
    mu_a, val_a = _pass(net, obs, dmu, dval)
    mu_b, val_b = _pass(plain, obs, dmu, dval)
    assert mu_a.shape == (ROWS, A) and mu_a.abs().max() > 0 and net.grad.abs().max() > 0
    assert torch.equal(mu_a, mu_b) and torch.equal(val_a, val_b)
    assert torch.equal(net.grad, plain.grad)                                       # every gradient of the trained column and the critic
    ga, gb = net.named_gradients(), plain.named_gradients()
    assert torch.equal(ga[f"a2c_network.pnn.actors.{t}.4.weight"], gb["a2c_network.mu.weight"]) and len(ga) == len(gb)
    assert torch.equal(ga[f"a2c_network.pnn.actors.{t}.0.weight"], gb["a2c_network.actor_mlp.0.weight"])
    if not mixed_precision:
        with torch.no_grad():                                                      # and it is the twin's column: the plans' usual distance to torch
            want = twin.eval_actor(obs.cpu())[0]
        assert (mu_a.cpu() - want).abs().max() <= 5e-5 * want.abs().max()
    # one Adam step over the flat buffer: the trained column moves, nothing outside the flat buffer does
    before = net.state_dict()
    ea, es, sq, gn = torch.zeros_like(net.flat), torch.zeros_like(net.flat), torch.zeros(256, device=dev), torch.zeros(1, device=dev)
    K.sqnorm_partial(net.grad, net.n_flat, sq)
    K.adam_step(net.flat, net.grad, ea, es, net.n_flat, lr=1e-3, step=1, max_norm=50.0, sqnorm_partials=sq, grad_norm_out=gn)
    after = net.state_dict()
    for k, v in carried.items():
        assert torch.equal(net.carried[k], v) and torch.equal(after[k], before[k]), k
    for k in before:
        if f".actors.{t}." in k or ".critic_mlp." in k or ".value." in k:
            assert not torch.equal(after[k], before[k]), k


# --------------------------------------------------------------------------------------------------------------------- 2. laterals
@pytest.mark.parametrize("activation", ["relu", "silu"])
@pytest.mark.parametrize("training_prim", [1, 2])
def test_lateral_column_forward_and_gradients_against_the_twin(dev, training_prim, activation):
    units, t = [36, 32], training_prim                                             # the concatenated second layer reads 72 / 108 columns
    torch.manual_seed(40 + t)
    twin = M.PnnTwin(OBS, units, A, P, t, has_lateral=True, activation=activation).jitter_biases()
    model = NP.AMPPNNLateralModel(_params(units, activation), actions_num=A, self_obs_size=20, task_obs_size=OBS - 20,
                                  task_obs_size_detail=_detail(t, True), device=dev)
    sd = twin.state_dict_ref()
    model.load_state_dict(sd)
    back = model.state_dict()
    assert all(torch.equal(back[k].cpu(), v) for k, v in sd.items()) and set(back) == set(sd)
    g = torch.Generator().manual_seed(10 + t)
    obs = torch.randn(ROWS, OBS, generator=g).clamp(-5, 5)
    wm, wv = torch.randn(ROWS, A, generator=g), torch.randn(ROWS, 1, generator=g)
    ws = model.workspace(ROWS, train=True)
    assert ws["g"].act_bufs["h1all"].shape[1] == (t + 1) * 36
    ws["x"].zero_()
    ws["x"][:, :OBS] = obs.to(dev)
    model.forward(ws, ROWS)
    mu_r, sigma_r = twin.eval_actor(obs)
    val_r = twin.eval_critic(obs)
    rel = lambda a, b: (a.detach().cpu().double() - b.detach().double()).abs().max().item() / (b.detach().double().abs().max().item() + 1e-12)
    e_mu, e_val = rel(ws["mu"], mu_r), rel(ws["val"], val_r)
    print(f"[pnn-lateral] t={t} {activation}: mu {e_mu:.3g} value {e_val:.3g}")
    assert ws["mu"].shape == (ROWS, A) and e_mu <= 5e-5 and e_val <= 5e-5
    assert torch.equal(model.sigma.cpu(), sigma_r[0].detach())
    ((mu_r * wm).sum() + (val_r * wv).sum()).backward()
    ws["dmu"].copy_(wm.to(dev))
    ws["dval"].copy_(wv.to(dev))
    model.book.grad.fill_(3.0)                                                     # stale values: the pass must overwrite every parameter's gradient
    model.backward(ws, ROWS)
    grads = model.net.gradients()
    seen, worst = [], 0.0
    for name, p in twin.named_parameters():
        if name.endswith(".sigma"):
            continue
        got = grads[name].reshape(p.shape)
        if p.grad is None:                                                         # frozen, or not evaluated (eval_actor, :62-89)
            assert (got == 0).all(), name
            continue
        assert p.grad.abs().max() > 0, name
        e = rel(got, p.grad)
        worst = max(worst, e)
        assert e <= 3e-4, (name, e)
        seen.append(name)
    print(f"[pnn-lateral] t={t} {activation}: worst gradient {worst:.3g} over {len(seen)} tensors")
    want = [f"a2c_network.critic_mlp.{i}.{q}" for i in (0, 2) for q in ("weight", "bias")] + ["a2c_network.value.weight", "a2c_network.value.bias"] + \
        [f"a2c_network.pnn.actors.{t}.{i}.{q}" for i in (0, 2, 4) for q in ("weight", "bias")] + [f"a2c_network.pnn.u.{t - 1}.{j}.0.weight" for j in range(t)]
    assert sorted(seen) == sorted(want)
    assert (model.book.grad[model.book._n:] == 0).all()


# --------------------------------------------------------------------------------------------------------------------- 3. agents
def _train_and_compare(agent, epochs=2):
    m = agent.model
    t = m.training_prim
    before = m.state_dict()
    disc_before = agent.disc.state_dict()
    for _ in range(epochs):
        info = agent.train_epoch()
        for key in ("actor_loss", "critic_loss", "disc_loss"):
            assert torch.isfinite(torch.stack(info[key])).all(), key
    after = m.state_dict()
    assert torch.isfinite(m.flat).all()
    moved = lambda k: f".pnn.actors.{t}." in k or ".critic_mlp." in k or ".value." in k or (getattr(m, "has_lateral", False) and t > 0 and f".pnn.u.{t - 1}." in k and k.endswith(".0.weight"))
    for k in before:
        if moved(k):
            if k.endswith(".weight"):
                assert not torch.equal(before[k], after[k]), k
        else:
            assert torch.equal(before[k], after[k]), k                              # every other column, a2c_network.mu.*, sigma
    assert any(not torch.equal(v, agent.disc.state_dict()[k]) for k, v in disc_before.items())
    return before, after


def test_agent_pnn_small_trains_one_column(dev):
    agent, _ = configs.make_agent("pnn_small", device=str(dev), seed=5)
    assert isinstance(agent.model, NP.AMPPNNNetwork) and (agent.model.num_prim, agent.model.training_prim) == (4, 0) and agent.actions_num == 69
    before, _ = _train_and_compare(agent)
    assert sum(".pnn.actors." in k for k in before) == 4 * 6 and "a2c_network.actor_mlp.0.weight" not in before


def test_agent_pnn_lateral_small_trains_one_column(dev):
    agent, _ = configs.make_agent("pnn_lateral_small", device=str(dev), seed=6)
    assert isinstance(agent.model, NP.AMPPNNLateralModel) and (agent.model.num_prim, agent.model.training_prim) == (3, 2)
    _train_and_compare(agent)
    with pytest.raises(NotImplementedError, match="mixed_precision"):
        configs.make_agent("pnn_lateral_small", device=str(dev), seed=6, mixed_precision=True)


@pytest.fixture(scope="module")
def trained(dev):
    """``pnn_small`` after one epoch on column 0, and its checkpoint."""
    agent, _ = configs.make_agent("pnn_small", device=str(dev), seed=7)
    agent.train_epoch()
    return agent, agent.get_full_state_weights()


def test_moving_on_to_the_next_primitive(dev, trained):
    agent0, state = trained
    assert state["training_prim"] == 0 and agent0.optimizer_step > 0 and agent0.exp_avg.abs().max() > 0
    nxt, _ = configs.make_agent("pnn_small", device=str(dev), seed=8, env_overrides={"training_prim": 1})
    assert nxt.model.training_prim == 1
    nxt.set_full_state_weights(state)
    got = nxt.model.state_dict()
    for k, v in state["model"].items():
        if "._disc_" not in k:
            assert torch.equal(got[k], v), k                                         # every column, the critic, a2c_network.mu.*
    for k, v in nxt.disc.state_dict().items():
        assert torch.equal(v, state["model"][k]), k
    assert torch.equal(nxt.running_mean_std.running_mean, agent0.running_mean_std.running_mean)
    assert torch.equal(nxt._amp_input_mean_std.running_var, agent0._amp_input_mean_std.running_var)
    assert nxt.optimizer_step == 0 and not nxt.exp_avg.any() and not nxt.exp_avg_sq.any()
    nxt.train_epoch()
    after = nxt.model.state_dict()
    for k, v in state["model"].items():
        if ".pnn.actors.0." in k:
            assert torch.equal(after[k], v), k                                       # the finished primitive is frozen
    assert not torch.equal(after["a2c_network.pnn.actors.1.0.weight"], state["model"]["a2c_network.pnn.actors.1.0.weight"])
    assert nxt.get_full_state_weights()["training_prim"] == 1
    # the same column again: the optimiser comes back as saved
    same, _ = configs.make_agent("pnn_small", device=str(dev), seed=9)
    same.set_full_state_weights(state)
    assert same.optimizer_step == state["optimizer"]["step"] and torch.equal(same.exp_avg, state["optimizer"]["exp_avg"])
    assert torch.equal(same.exp_avg_sq, state["optimizer"]["exp_avg_sq"]) and torch.equal(same.disc_exp_avg, state["disc_optimizer"]["exp_avg"])


def test_consumers_read_the_saved_checkpoint(dev, trained):
    """PnnTeacher and HumanoidImMCP take the agent's checkpoint unchanged.  Against the agent network's mu the teacher agrees to the teacher test's
    2e-5, not bit for bit: the teacher runs one MlpGraph GEMM per layer and column, the agent network the batched actor + critic plans and the
    skinny head kernel -- other tilings, other summation orders."""
    from pulse_amd.learning.teacher import PnnTeacher
    agent, state = trained
    n = agent.num_actors
    teacher = PnnTeacher(state, None, num_prim=4, num_envs=n, activation="relu", device=dev)
    assert (teacher.in_dim, teacher.num_actions) == (934, 69)
    obs = agent.vec_env.task.obs_buf
    x = teacher.normalize(obs)
    prim = teacher.primitives()[:, :, :69].clone()
    for k in range(4):
        net = agent.model if k == 0 else NP.AMPPNNNetwork(agent.config["network"], actions_num=69, input_shape=(934,),
                                                          task_obs_size_detail=_detail(k, False, 4), device=dev)
        if k:
            net.load_state_dict(state["model"])
        ws = net.workspace(n, train=False)
        net.eval()
        ws["x"].zero_()
        ws["x"][:, :934] = x[:, :934]
        net.forward(ws, n)
        assert ws["mu"].abs().max() > 0
        np.testing.assert_allclose(prim[:, k].cpu().numpy(), ws["mu"].cpu().numpy(), atol=2e-5, rtol=2e-5)
    assert not torch.equal(prim[:, 0], prim[:, 1])
    # the MCP env on the same checkpoint: its step blends what the twin's composition gives for these weights
    from pulse_amd import synthetic as syn
    from pulse_amd.env.humanoid_im_mcp import HumanoidImMCP
    from pulse_amd.env.motion_lib import MotionLib
    from pulse_amd.env.sim import PdSim
    env_cfg = dict(configs.ENV_IM, has_pnn=True, num_prim=4, has_lateral=False)
    motion = MotionLib.from_tables(syn.synthetic_motion_library(syn.make_generator(8, 0), 16), dev)
    task = HumanoidImMCP({"env": env_cfg}, PdSim(16, 17, dev, seed=3), motion, device=dev, pnn_checkpoint=state)
    task.reset()
    obs0 = task.obs_buf.clone()
    weights = torch.rand(16, 4, generator=torch.Generator().manual_seed(2)) * 2 - 0.5
    task.step(weights.to(dev))
    cpu = {"model": {k: v.cpu() for k, v in state["model"].items()}, "running_mean_std": {k: v.cpu() for k, v in state["running_mean_std"].items()}}
    want = MM.compose(cpu, 4, "relu", obs0.cpu(), weights)
    np.testing.assert_allclose(task.actions.cpu().numpy(), want.numpy(), atol=2e-5, rtol=2e-5)


def test_runner_builds_trains_and_plays_amp_pnn(dev, tmp_path):
    from pulse_amd import runner as R
    from tests.test_runner_cpu import im_params
    p = im_params()
    p["params"]["network"] = dict(configs.NETWORK_PNN, mlp=dict(configs.NETWORK_PNN["mlp"], units=[128, 64]),
                                  disc=dict(configs.NETWORK_PNN["disc"], units=[128, 64]))
    p["params"]["config"].update({"num_actors": 64, "horizon_length": 16, "minibatch_size": 256, "device": "cuda:0", "env_name": "pulse_pnn",
                                  "env_config": {"seed": 3}, "train_dir": str(tmp_path), "amp_minibatch_size": 64, "amp_obs_demo_buffer_size": 4096,
                                  "amp_replay_buffer_size": 4096, "amp_batch_size": 128})
    keys = {"num_prim": 3, "training_prim": 1, "actors_to_load": 1, "has_lateral": False}
    R.register_env("pulse_pnn", lambda num_actors, seed=0, **kw: configs.make_env(num_actors, 16, "cuda:0", seed=seed, env_kind="amp",
                                                                                  env_overrides=keys)[0])
    r = R.build_alg_runner()
    r.model_builder.network_factory.create("amp_pnn")                            # registered (run_hydra.py:261)
    r.load(p)
    r.run({"train": True, "max_epochs": 1})
    ag = r.agent
    assert isinstance(ag.model, NP.AMPPNNNetwork) and ag.epoch_num == 1 and (ag.model.num_prim, ag.model.training_prim) == (3, 1)
    ckpt = ag.get_full_state_weights()
    r2 = R.build_alg_runner()
    r2.load(p)
    player = r2.player_factory.create(r2.algo_name, config=r2.config)
    player.restore(ckpt)
    a = player.get_action(player.env.reset(), is_determenistic=True)
    assert a.shape == (64, 69) and torch.isfinite(a).all()
    for k, v in ag.model.state_dict().items():
        assert torch.equal(v, player.model.state_dict()[k]), k


# --------------------------------------------------------------------------------------------------------------------- 4. launch audit
@pytest.mark.parametrize("name,min_launches", [("pnn_small", 12), ("pnn_lateral_small", 20)])
def test_every_gemm_launch_of_an_epoch_matches_the_fp64_model(dev, auditor, monkeypatch, name, min_launches):  # noqa: F811
    monkeypatch.setattr(K, "F32_MODE", "x3")
    torch.manual_seed(7)
    agent, _ = configs.make_agent(name, device=str(dev), seed=7, mini_epochs=1)
    play = agent.play_steps

    def play_steps():
        auditor.phase = "rollout"
        try:
            return play()
        finally:
            auditor.phase = "update"
    monkeypatch.setattr(agent, "play_steps", play_steps)
    agent.train_epoch()
    torch.cuda.synchronize()
    rows = auditor.rows
    print(f"[audit-summary] {name}: {len(rows)} launches audited, worst err/tol {max(r['worst'] for r in rows):.3g}")
    assert not auditor.failures, "\n".join(auditor.failures[:20])
    assert len(rows) >= min_launches
    phases = {(r["phase"], r["form"]) for r in rows}
    assert ("rollout", "fwd") in phases and ("update", "fwd") in phases and ("update", "dx") in phases and ("update", "dw") in phases, phases
    if name == "pnn_lateral_small":                                               # the concatenated second layer: K = 3 x 36, and its slice-only input gradient
        assert any(r["form"] == "fwd" and r["K"] == 108 and r["N"] == 32 for r in rows)
        assert any(r["form"] == "dx" and r["N"] == 36 and r["K"] == 32 for r in rows)
        assert any(r["form"] == "dw" and r["M"] == 32 and r["N"] == 108 for r in rows)
