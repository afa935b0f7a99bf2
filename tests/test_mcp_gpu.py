"""GPU: PHC's MCP composer stage on the HIP path -- pulse_mcp_compose / pulse_mcp_head_forward / pulse_mcp_head_backward (csrc/mcp.hip) against
fp64 models, the amp_mcp network against the plain-torch twin's autograd (tests/mcp_model.py, itself held to the reference bit for bit by
tests/test_mcp_cpu.py), HumanoidImMCP / HumanoidImMCPGetup against the twin's composition and a plain HumanoidIm, and the agent end to end.

Bounds (u = 2^-24, 2u = 2^-23):
  compose      per element  P * 2^-23 * sum_k |w_k x_k|: P rounded products and a (P - 1)-term fp32 sum in any order
  softmax      absolute     (P + 8) * 2^-23 on outputs <= 1: rounding of the shifted argument, an exp good to a few ulp, a P-term sum, a division
  softmax bwd  per element  (P + 4) * 2^-23 * mu_j (|dmu_j| + sum_k |mu_k dmu_k|) * max(1, |act'|), + 2^-126 where fp32 underflows
  SiLU'        1e-6 of the gradient it multiplies, on the derivative's own scale max(1, |act'|) (act' lies in [-0.1, 1.1] and crosses zero at
               z = -1.278, where no fp32 evaluation of s (1 + z (1 - s)) has a relative error); ReLU is exact
"""
import ctypes

import numpy as np
import pytest
import torch

from pulse_amd import _lib, configs, kernels as K, ops
from pulse_amd import synthetic as syn
from pulse_amd._lib import ACT_NONE, ACT_RELU, ACT_SILU, ACT_SILU_D
from tests import mcp_model as M

pytestmark = pytest.mark.gpu

U2 = 2.0 ** -23
TINY = 2.0 ** -126                                                               # the smallest normal fp32
SENT = 7.25


def _pitched(t, extra, dev):
    """``t`` (rows, cols) as a non-contiguous view of a wider buffer whose other columns hold a sentinel."""
    buf = torch.full((t.shape[0], t.shape[1] + extra), SENT, device=dev)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf, buf[:, :t.shape[1]]


# --------------------------------------------------------------------------------------------------------------------- 1. compose
@pytest.mark.parametrize("P", [1, 3, 4, 32])
def test_compose_against_fp64_model(dev, P):
    g = torch.Generator().manual_seed(100 + P)
    for N in (1, 63, 64, 65, 257):
        for A in (5, 69):
            ap = (A + 3) // 4 * 4
            w = torch.randn(N, P, generator=g)
            x = torch.randn(N, P, ap, generator=g) * 3
            wbuf, wv = _pitched(w, 3, dev)
            xbuf, _ = _pitched(x.reshape(N, P * ap), 8, dev)
            xv = xbuf.as_strided((N, P, ap), (xbuf.stride(0), ap, 1))
            obuf = torch.full((N, A + 3), SENT, device=dev)
            got = ops.mcp_compose(wv, xv, obuf[:, :A], num_actions=A)
            assert got.shape == (N, A) and got.data_ptr() == obuf.data_ptr()
            prod = w.double()[:, :, None] * x.double()[:, :, :A]
            ref, bound = prod.sum(1), P * U2 * prod.abs().sum(1)
            err = (got.cpu().double() - ref).abs()
            assert (err <= bound).all(), (N, P, A, (err - bound).max().item())
            assert (obuf[:, A:] == SENT).all() and (wbuf[:, P:] == SENT).all() and (xbuf[:, P * ap:] == SENT).all()
            # discrete_moe: one_hot(argmax) of the weights, exactly
            if P > 1:
                assert (w.sort(dim=1).values.diff(dim=1) > 0).all()                      # no ties in the draw
            obuf.fill_(SENT)
            got = ops.mcp_compose(wv, xv, obuf[:, :A], num_actions=A, discrete=True)
            hot = torch.nn.functional.one_hot(w.argmax(1), num_classes=P).float()
            want = torch.sum(hot[:, :, None] * x[:, :, :A], dim=1)
            assert torch.equal(got.cpu(), want), (N, P, A)
            assert torch.equal(got.cpu(), x[torch.arange(N), w.argmax(1), :A] + 0.0)
            assert (obuf[:, A:] == SENT).all()


def test_compose_negative_and_zero_weight_rows(dev):
    x = torch.randn(3, 3, 72, generator=torch.Generator().manual_seed(4))
    w = torch.tensor([[0.0, 0.0, 0.0], [-0.5, -0.25, -2.0], [0.3, -0.7, 0.1]])
    got = ops.mcp_compose(w.to(dev), x.to(dev), num_actions=69).cpu()
    prod = w.double()[:, :, None] * x.double()[:, :, :69]
    assert (got[0] == 0).all()
    assert ((got.double() - prod.sum(1)).abs() <= 3 * U2 * prod.abs().sum(1)).all()
    got = ops.mcp_compose(w.to(dev), x.to(dev), num_actions=69, discrete=True).cpu()
    assert torch.equal(got, x[torch.arange(3), torch.tensor([0, 1, 0]), :69] + 0.0)      # a zero row: argmax is its FIRST maximum


def test_mcp_argument_errors(dev):
    lib = _lib.load()
    t = torch.zeros(4, 128, device=dev)
    p, s = ctypes.c_void_p(t.data_ptr()), None
    bad = [lambda: lib.pulse_mcp_compose(None, 4, p, 128, 8, 4, 4, 5, 0, p, 8, s),                  # null pointer
           lambda: lib.pulse_mcp_compose(p, 4, p, 128, 8, 4, 0, 5, 0, p, 8, s),                     # num_prim 0
           lambda: lib.pulse_mcp_compose(p, 33, p, 1024, 8, 4, 33, 5, 0, p, 8, s),                  # num_prim 33
           lambda: lib.pulse_mcp_compose(p, 3, p, 128, 8, 4, 4, 5, 0, p, 8, s),                     # w_stride < num_prim
           lambda: lib.pulse_mcp_compose(p, 4, p, 128, 4, 4, 4, 5, 0, p, 8, s),                     # a_pitch < num_actions
           lambda: lib.pulse_mcp_compose(p, 4, p, 31, 8, 4, 4, 5, 0, p, 8, s),                      # x_stride < num_prim * a_pitch
           lambda: lib.pulse_mcp_compose(p, 4, p, 128, 8, 4, 4, 5, 0, p, 4, s),                     # actions_stride < num_actions
           lambda: lib.pulse_mcp_compose(p, 4, p, 128, 8, -1, 4, 5, 0, p, 8, s),
           lambda: lib.pulse_mcp_head_forward(None, 4, 4, 4, p, 4, s),
           lambda: lib.pulse_mcp_head_forward(p, 4, 4, 33, p, 4, s),
           lambda: lib.pulse_mcp_head_forward(p, 3, 4, 4, p, 4, s),
           lambda: lib.pulse_mcp_head_backward(p, 4, None, 0, None, 0, ACT_NONE, 4, 4, None, 4, s),
           lambda: lib.pulse_mcp_head_backward(p, 4, None, 0, None, 0, ACT_RELU, 4, 4, p, 4, s),    # the derivative needs aux
           lambda: lib.pulse_mcp_head_backward(p, 4, p, 3, None, 0, ACT_NONE, 4, 4, p, 4, s),
           lambda: lib.pulse_mcp_head_backward(p, 4, None, 0, None, 0, 9, 4, 4, p, 4, s),
           lambda: lib.pulse_mcp_head_backward(p, 4, None, 0, None, 0, ACT_NONE, 4, 0, p, 4, s)]
    for i, f in enumerate(bad):
        assert f() == -1, i
        assert lib.pulse_last_error().startswith(b"pulse_mcp_"), i
    # N = 0 is a no-op, null pointers included
    assert lib.pulse_mcp_compose(None, 0, None, 0, 0, 0, 4, 5, 0, None, 0, s) == 0
    assert lib.pulse_mcp_head_forward(None, 0, 0, 4, None, 0, s) == 0
    assert lib.pulse_mcp_head_backward(None, 0, None, 0, None, 0, ACT_RELU, 0, 4, None, 0, s) == 0
    assert ops.mcp_compose(torch.zeros(0, 4, device=dev), torch.zeros(0, 4, 8, device=dev), num_actions=5).shape == (0, 5)
    # the wrappers reject what the kernels would re-interpret
    w, x = torch.zeros(4, 4, device=dev), torch.zeros(4, 4, 8, device=dev)
    with pytest.raises(ValueError):
        ops.mcp_compose(w.cpu(), x)
    with pytest.raises(TypeError):
        ops.mcp_compose(w.double(), x)
    with pytest.raises(ValueError):
        ops.mcp_compose(w.t(), x)
    with pytest.raises(ValueError):
        ops.mcp_compose(w, x.transpose(1, 2))
    with pytest.raises(ValueError):
        ops.mcp_compose(w, x, num_actions=9)
    with pytest.raises(TypeError):
        K.mcp_head_forward(w.cpu(), w, rows=4, num_prim=4)
    with pytest.raises(TypeError):
        K.mcp_head_forward(w.double(), w, rows=4, num_prim=4)
    with pytest.raises(ValueError):
        K.mcp_head_forward(w.t(), w, rows=4, num_prim=4)
    with pytest.raises(ValueError):
        K.mcp_head_backward(w, w.clone(), rows=4, num_prim=5)
    with pytest.raises(ValueError):
        K.mcp_head_backward(w, w.clone(), rows=4, num_prim=4, activation=ACT_RELU)


# --------------------------------------------------------------------------------------------------------------------- 2. head
def _silu_d64(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


@pytest.mark.parametrize("P", [1, 3, 4, 32])
@pytest.mark.parametrize("N", [1, 64, 65, 300])
def test_head_forward_and_backward_against_fp64(dev, N, P):
    g = torch.Generator().manual_seed(1000 * P + N)
    h = torch.randn(N, P, generator=g) * 2
    big = torch.rand(N, P, generator=g) < 0.15                                   # logits up to +-80 next to ordinary ones
    h = torch.where(big, (torch.rand(N, P, generator=g) * 160 - 80), h)
    hbuf, hv = _pitched(h, 5, dev)
    mbuf = torch.full((N, P + 2), SENT, device=dev)
    mu = K.mcp_head_forward(hv, mbuf[:, :P], rows=N, num_prim=P)[:, :P]
    ref = torch.softmax(h.double(), dim=1)
    err = (mu.cpu().double() - ref).abs().max().item()
    assert err <= (P + 8) * U2, (N, P, err)
    assert (mbuf[:, P:] == SENT).all() and (hbuf[:, P:] == SENT).all()
    # backward with the kernel's own mu
    mu64 = mu.cpu().double()
    dmu = torch.randn(N, P, generator=g)
    z = torch.randn(N, P, generator=g) * 2                                       # the last Linear's output (for the activation's derivative)
    dbuf, dv = _pitched(dmu, 1, dev)
    dot = (mu64 * dmu.double()).sum(1, keepdim=True)
    dh = mu64 * (dmu.double() - dot)
    soft_bound = (P + 4) * U2 * mu64 * (dmu.double().abs() + (mu64 * dmu.double()).abs().sum(1, keepdim=True))
    d64 = _silu_d64(z.double())
    cases = [(True, ACT_NONE, None, torch.ones_like(dh)), (True, ACT_RELU, z.clamp(min=0), (z > 0).double()), (True, ACT_SILU, z, d64),
             (True, ACT_SILU_D, d64.float(), d64.float().double()),
             (False, ACT_NONE, None, torch.ones_like(dh)), (False, ACT_RELU, z.clamp(min=0), (z > 0).double()), (False, ACT_SILU, z, d64)]
    for softmax, act, aux, deriv in cases:
        zbuf = torch.full((N, P + 3), SENT, device=dev)
        auxv = _pitched(aux, 2, dev)[1] if aux is not None else None
        got = K.mcp_head_backward(dv, zbuf[:, :P], rows=N, num_prim=P, mu=mbuf[:, :P] if softmax else None, aux=auxv, activation=act)
        got = got[:, :P].cpu()
        assert (zbuf[:, P:] == SENT).all()
        base = dh if softmax else dmu.double()
        want = base * deriv
        scale = deriv.abs().clamp(min=1.0)
        # (TINY: fp32 cannot hold a product below its smallest normal to relative accuracy -- a softmax output next to a logit 80 above it is
        #  of that size; the floor covers gradual underflow and a flush to zero alike)
        bound = (soft_bound * scale + TINY if softmax else torch.zeros_like(want))
        if act == ACT_SILU:
            bound = bound + 1e-6 * base.abs() * scale
        elif act == ACT_SILU_D:
            bound = bound + 2.0 ** -24 * want.abs()                              # one rounded product with the stored derivative
        if not softmax and act in (ACT_NONE, ACT_RELU):
            assert torch.equal(got.double(), want), (N, P, softmax, act)         # dz is dmu or 0
        else:
            e = (got.double() - want).abs()
            assert (e <= bound).all(), (N, P, softmax, act, (e - bound).max().item())


# --------------------------------------------------------------------------------------------------------------------- 3. network
def _net_params(units, activation, has_softmax):
    p = {"name": "amp_mcp", "separate": True, "ending_act": True,
         "space": {"continuous": {"sigma_init": {"name": "const_initializer", "val": -2.9}, "fixed_sigma": True}},
         "mlp": {"units": list(units), "activation": activation}}
    if has_softmax is not None:
        p["has_softmax"] = has_softmax
    return p


@pytest.mark.parametrize("P", [3, 4])
@pytest.mark.parametrize("activation", ["relu", "silu"])
@pytest.mark.parametrize("has_softmax", [False, True])
def test_amp_mcp_forward_and_gradients_against_the_twin(dev, has_softmax, activation, P):
    from pulse_amd.learning.network_mcp import AMPMCPModel
    torch.manual_seed(6 + P)
    m = 300
    twin = M.McpTwin(934, [96, 64], P, activation=activation, has_softmax=has_softmax)
    with torch.no_grad():
        for p in twin.parameters():
            if p.dim() == 1 and p.requires_grad:
                p.add_(0.1 * torch.randn_like(p))
    model = AMPMCPModel(_net_params([96, 64], activation, has_softmax), actions_num=P, self_obs_size=358, task_obs_size=576,
                        task_obs_size_detail={"num_prim": P}, device=dev)
    assert model.in_pitch == 960 and model.net.has_softmax == has_softmax
    sd = twin.state_dict_ref()
    model.load_state_dict(sd)
    back = model.state_dict()
    assert [k for k in back if k != "a2c_network.sigma"] == [k for k, _ in twin.layout()]
    for k, v in sd.items():
        assert torch.equal(back[k].cpu(), v), k
    obs = torch.randn(m, 934).clamp(-5, 5)
    ws = model.workspace(m, train=True)
    ws["x"].zero_()
    ws["x"][:, :934] = obs.to(dev)
    model.forward(ws, m)
    mu_r, sigma_r = twin.eval_actor(obs)
    val_r = twin.eval_critic(obs)
    rel = lambda a, b: (a.detach().cpu().double() - b.detach().double()).abs().max().item() / (b.detach().double().abs().max().item() + 1e-12)
    assert ws["mu"].shape == (m, P) and rel(ws["mu"], mu_r) <= 5e-5 and rel(ws["val"], val_r) <= 5e-5
    assert torch.equal(model.sigma.cpu(), sigma_r[0].detach())
    wm, wv = torch.randn(m, P), torch.randn(m, 1)
    ((mu_r * wm).sum() + (val_r * wv).sum()).backward()
    ws["dmu"].copy_(wm.to(dev))
    ws["dval"].copy_(wv.to(dev))
    model.book.grad.fill_(3.0)                                                  # stale values: the pass must overwrite every parameter's gradient
    model.backward(ws, m)
    grads = model.net.gradients()
    seen = 0
    for name, p in twin.named_parameters():
        if name.endswith(".sigma"):
            continue
        got = grads[name].reshape(p.shape)
        if ".actor_mlp." in name or ".mu." in name:
            assert p.grad is None and (got == 0).all(), name                   # never evaluated (eval_actor, :64-86)
            continue
        assert p.grad is not None and p.grad.abs().max() > 0, name
        assert rel(got, p.grad) <= 3e-4, name
        seen += 1
    assert seen == 2 * (3 + 3)                                                  # composer (3 layers) + critic (2 layers + value), weight and bias


def test_amp_mcp_defaults_and_refusals(dev):
    from pulse_amd.learning.network_mcp import AMPMCPNetwork
    kw = dict(self_obs_size=20, task_obs_size=12, device=dev)
    net = AMPMCPNetwork(_net_params([16, 8], "relu", None), actions_num=4, task_obs_size_detail={}, **kw)
    assert net.has_softmax is True and net.num_prim == 4                        # amp_network_mcp_builder.py:33, :39
    with pytest.raises(ValueError, match="num_prim"):
        AMPMCPNetwork(_net_params([16, 8], "relu", False), actions_num=69, task_obs_size_detail={"num_prim": 4}, **kw)


# --------------------------------------------------------------------------------------------------------------------- 4. env
def _mcp_env(dev, cls_name="HumanoidImMCP", n=16, seed=3, has_lateral=False, plain=False, **env_over):
    from pulse_amd.env import humanoid_im_mcp as H
    from pulse_amd.env.humanoid_im import HumanoidIm
    from pulse_amd.env.motion_lib import MotionLib
    from pulse_amd.env.sim import PdSim
    env_cfg = dict(configs.ENV_IM, has_pnn=True, num_prim=4, has_lateral=has_lateral, **env_over)
    motion = MotionLib.from_tables(syn.synthetic_motion_library(syn.make_generator(seed + 5, 0), n), dev)
    sim = PdSim(n, 17, dev, seed=seed)                                         # the action-dependent physics stand-in
    if plain:
        return HumanoidIm({"env": env_cfg}, sim, motion, device=dev), None
    ck = syn.synthetic_pnn_checkpoint(4, in_dim=934, seed=9, has_lateral=has_lateral)
    return getattr(H, cls_name)({"env": env_cfg}, sim, motion, device=dev, pnn_checkpoint=ck), ck


def test_env_step_composes_the_primitives_and_steps_like_humanoid_im(dev):
    from pulse_amd.env.humanoid_im import VecTaskPythonWrapper
    task, ck = _mcp_env(dev)
    plain, _ = _mcp_env(dev, plain=True)
    env = VecTaskPythonWrapper(task, rl_device=dev)
    assert task.num_actions == 4 and env.num_actions == 4 and env.get_env_info()["action_space"].shape == (4,)
    assert task.get_task_obs_size_detail()["num_prim"] == 4 and "num_prim" not in plain.get_task_obs_size_detail()
    assert plain.num_actions == 69 and task.num_obs == plain.num_obs == 934
    task.reset()
    plain.reset()
    assert torch.equal(task.obs_buf, plain.obs_buf)
    weights = torch.rand(16, 4, generator=torch.Generator().manual_seed(2)) * 2 - 0.5
    for _ in range(2):
        obs0 = task.obs_buf.clone()
        task.step(weights.to(dev))
        want = M.compose(ck, 4, "relu", obs0.cpu(), weights)
        np.testing.assert_allclose(task.actions.cpu().numpy(), want.numpy(), atol=2e-5, rtol=2e-5)
        assert task.actions.shape == (16, 69)
        plain.step(task.actions.clone())
        for a, b in ((task.obs_buf, plain.obs_buf), (task.rew_buf, plain.rew_buf), (task.reset_buf, plain.reset_buf),
                     (task.progress_buf, plain.progress_buf), (task.sim.dof_pos, plain.sim.dof_pos)):
            assert torch.equal(a, b)
    assert torch.isfinite(task.obs_buf).all() and task.rew_buf.abs().sum().item() > 0


def test_env_discrete_moe_picks_one_primitive(dev):
    task, ck = _mcp_env(dev, discrete_moe=True)
    task.reset()
    obs0 = task.obs_buf.clone()
    weights = torch.rand(16, 4, generator=torch.Generator().manual_seed(8))
    task.step(weights.to(dev))
    x_all = task._pnn.g.act_bufs["acts"].view(16, 4, 72)
    pick = x_all[torch.arange(16, device=dev), weights.argmax(1).to(dev), :69]
    assert torch.equal(task.actions, pick + 0.0)
    want = M.compose(ck, 4, "relu", obs0.cpu(), weights, discrete=True)
    np.testing.assert_allclose(task.actions.cpu().numpy(), want.numpy(), atol=2e-5, rtol=2e-5)


def test_env_lateral_primitives(dev):
    task, ck = _mcp_env(dev, has_lateral=True, z_activation="silu")
    task.reset()
    obs0 = task.obs_buf.clone()
    weights = torch.rand(16, 4, generator=torch.Generator().manual_seed(12))
    task.step(weights.to(dev))
    want = M.compose(ck, 4, "silu", obs0.cpu(), weights, has_lateral=True)
    np.testing.assert_allclose(task.actions.cpu().numpy(), want.numpy(), atol=2e-5, rtol=2e-5)


def test_mcp_getup_env_constructs_and_keeps_its_recovery_bookkeeping(dev):
    from pulse_amd.env import humanoid_im_mcp as H
    from pulse_amd.env.humanoid_im_getup import HumanoidImGetup
    env, _ = configs.make_env(16, 16, str(dev), seed=4, env_kind="mcp")
    task = env.task
    assert isinstance(task, H.HumanoidImMCPGetup) and isinstance(task, HumanoidImGetup) and isinstance(task, H.HumanoidImMCP)
    assert task.num_actions == 4 and env.get_env_info()["action_space"].shape == (4,) and task.get_task_obs_size_detail()["num_prim"] == 4
    assert task._pnn.in_dim == task.num_obs and task.models_path and isinstance(task.models_path[0], dict)
    env.reset()
    task.update_getup_schedule(0, task.getup_udpate_epoch)                       # before the schedule's epoch: every reset is a fall start
    assert (task._recovery_episode_prob, task._fall_init_prob) == (0.0, 1.0)
    task._recovery_counter[:5] = 3
    prog = task.progress_buf.clone()
    obs, rew, reset, _ = env.step(torch.rand(16, 4, device=dev))
    assert obs.shape == (16, task.num_obs) and torch.isfinite(obs).all() and torch.isfinite(rew).all()
    assert (task._recovery_counter[:5] == 2).all() and (reset[:5] == 0).all()   # in recovery: no reset, the counter runs down (:198-210)
    assert torch.equal(task.progress_buf[:5], prog[:5]) and (task.progress_buf[5:] >= prog[5:]).all()
    assert task.actions.shape == (16, 69)
    env.reset_masked(torch.ones(16, dtype=torch.bool, device=dev))
    assert (task._recovery_counter == task._recovery_steps).all()               # fall starts get recoverySteps of grace (:137-165)


# --------------------------------------------------------------------------------------------------------------------- 5. agent
def _mu_of(agent, obs):
    n = obs.shape[0]
    ws = agent.model.workspace(n, train=False)
    agent.set_eval()
    agent._preproc_obs(obs, ws, n)
    agent.model.forward(ws, n)
    return ws["mu"].clone()


def test_agent_trains_the_composer_and_leaves_the_unused_heads_alone(dev):
    agent, _ = configs.make_agent("mcp_small", device=str(dev), seed=5)
    from pulse_amd.learning.network_mcp import AMPMCPModel
    assert isinstance(agent.model, AMPMCPModel) and agent.actions_num == 4 and not agent.model.net.has_softmax
    before = agent.model.state_dict()
    for _ in range(2):
        info = agent.train_epoch()
        for key in ("actor_loss", "critic_loss"):
            assert torch.isfinite(torch.stack(info[key])).all(), key
    after = agent.model.state_dict()
    assert torch.isfinite(agent.model.flat).all()
    for k in before:
        if ".actor_mlp." in k or ".mu." in k or k.endswith(".sigma"):
            assert torch.equal(before[k], after[k]), k                           # zero gradient: bit-identical
        elif k.endswith(".weight"):
            assert not torch.equal(before[k], after[k]), k                       # composer and critic move
    # a second agent restored from the checkpoint reproduces mu bit for bit
    state = agent.get_full_state_weights()
    assert "a2c_network.composer.4.weight" in state["model"] and "a2c_network.actor_mlp.0.weight" in state["model"]
    other, _ = configs.make_agent("mcp_small", device=str(dev), seed=77)
    other.set_full_state_weights(state)
    obs = agent.vec_env.task.obs_buf
    other.vec_env.task.obs_buf.copy_(obs)
    mu_a, mu_b = _mu_of(agent, obs), _mu_of(other, other.vec_env.task.obs_buf)
    assert mu_a.shape == (64, 4) and torch.equal(mu_a, mu_b)
    with pytest.raises(NotImplementedError, match="amp_mcp"):
        configs.make_agent("mcp_small", device=str(dev), seed=5, mixed_precision=True)


def test_runner_builds_trains_and_plays_amp_mcp(dev, tmp_path):
    from pulse_amd import runner as R
    from tests.test_runner_cpu import im_params
    p = im_params()
    p["params"]["network"] = dict(configs.NETWORK_MCP, mlp=dict(configs.NETWORK_MCP["mlp"], units=[128, 64]),
                                  disc=dict(configs.NETWORK_MCP["disc"], units=[128, 64]))
    p["params"]["config"].update({"num_actors": 64, "horizon_length": 16, "minibatch_size": 256, "device": "cuda:0", "env_name": "pulse_mcp",
                                  "env_config": {"seed": 3}, "train_dir": str(tmp_path)})
    R.register_env("pulse_mcp", lambda num_actors, seed=0, **kw: configs.make_env(num_actors, 16, "cuda:0", seed=seed, env_kind="mcp")[0])
    r = R.build_alg_runner()
    r.model_builder.network_factory.create("amp_mcp")                            # registered (run_hydra.py:262)
    r.load(p)
    r.run({"train": True, "max_epochs": 1})
    ag = r.agent
    from pulse_amd.learning.network_mcp import AMPMCPModel
    assert isinstance(ag.model, AMPMCPModel) and ag.epoch_num == 1
    ckpt = ag.get_full_state_weights()
    r2 = R.build_alg_runner()
    r2.load(p)
    player = r2.player_factory.create(r2.algo_name, config=r2.config)
    player.restore(ckpt)
    a = player.get_action(player.env.reset(), is_determenistic=True)
    assert a.shape == (64, 4) and torch.isfinite(a).all()
    for k, v in ag.model.state_dict().items():
        assert torch.equal(v, player.model.state_dict()[k]), k
