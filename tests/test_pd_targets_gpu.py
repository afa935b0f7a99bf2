"""GPU: the actuation launch (pulse_pd_targets, csrc/pd_targets.hip) and the envs that call it against tests/pd_targets_model.py.

Every operation of the stage is exact or correctly rounded and runs in the model's order (the product rounded before the sum), so every output
is compared BIT FOR BIT; a NaN must sit where the model has one.
  kernel   N in {1, 5, 33} x D in {69, 153}, plain and residual form, clip 1 and inf, no freeze / the first joint / the last joint, contiguous and
           padded row pitches with poison behind the written columns, NaN / +-inf actions (and NaN poses in the residual form); the 16-byte form
           at D = 72 with aligned pitches, and its fall-back when a base address is not aligned; the clamped copy written in place;
  env      with published limits and each cfg.robot switch on, sim.pd_targets after a step equals the model (24 and 52 bodies, res_action, a
           downstream task); with no limits and no switches the targets are clamp(actions); the stage is ONE launch and no clamp / addcmul.
"""
import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import pd_targets_model as M
from pulse_amd import configs, ops
from pulse_amd import synthetic as syn

pytestmark = pytest.mark.gpu

POISON = 1234.5


def assert_same_bits(got, want, what):
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan), f"{what}: NaNs are not where the model has them"
    g, w = got.view(torch.int32)[~nan], want.view(torch.int32)[~nan]
    bad = int((g != w).sum())
    assert bad == 0, f"{what}: {bad} of {w.numel()} elements differ in their bits"


def _tables(d, g):
    scale = (0.3 + 3.0 * torch.rand(d, generator=g))
    scale[4] = 5.0
    offset = torch.where(torch.rand(d, generator=g) < 0.5, torch.randn(d, generator=g), torch.zeros(d))
    return offset, scale


def _inputs(n, d, seed, specials=True):
    g = torch.Generator().manual_seed(seed)
    a = M.ACTION_SIGMA * torch.randn(n, d, generator=g)
    ref = M.POSE_SIGMA * torch.randn(n, d, generator=g)
    sim = ref + M.POSE_SIGMA * torch.randn(n, d, generator=g)
    if specials:
        flat = a.view(-1)
        for i, v in enumerate((float("nan"), float("inf"), float("-inf"), -0.0, 1.0, -1.0)):
            flat[(7 * i + 3) % flat.numel()] = v
        ref.view(-1)[(11 + d) % ref.numel()] = float("nan")
        sim.view(-1)[(23 + d) % sim.numel()] = float("nan")
    return a, ref, sim, g


def _pitched(t, pad, dev, fill=0.0):
    """``t`` as the first columns of a wider device buffer (row pitch = columns + pad), the rest filled with ``fill``."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=torch.float32, device=dev)
    buf[:, :t.shape[1]] = t.to(dev)
    return buf, buf[:, :t.shape[1]]


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("d", [69, 153])
@pytest.mark.parametrize("n", [1, 5, 33])
def test_kernel_equals_the_model(dev, n, d, res):
    a, ref, sim, g = _inputs(n, d, 100 * n + d)
    offset, scale = _tables(d, g)
    first, last = torch.zeros(d, dtype=torch.bool), torch.zeros(d, dtype=torch.bool)
    first[0:3], last[d - 3:d] = True, True
    assert 0.2 <= float((a.abs() > 1).float().mean()) <= 0.8 or n == 1
    for clip in (1.0, float("inf")):
        for fz in (None, first, last):
            for pad in (0, 3):
                want_a, want_t = M.targets(a, clip, offset, scale, fz, ref if res else None, sim if res else None)
                _, av = _pitched(a, pad, dev)
                _, rv = _pitched(ref, 2 * pad, dev)
                _, sv = _pitched(sim, pad, dev)
                cbuf, cv = _pitched(torch.full((n, d), POISON), pad + 1 if pad else 0, dev, POISON)
                tbuf, tv = _pitched(torch.full((n, d), POISON), pad, dev, POISON)
                got_a, got_t = ops.pd_targets(av, scale.to(dev), clip=clip, offset=offset.to(dev), freeze=None if fz is None else fz.to(dev),
                                              ref_dof_pos=rv if res else None, sim_dof_pos=sv if res else None, clamped=cv, target=tv)
                what = f"n={n} d={d} res={res} clip={clip} freeze={'none' if fz is None else int(fz.nonzero()[0])} pad={pad}"
                assert got_a.data_ptr() == cbuf.data_ptr() and got_t.data_ptr() == tbuf.data_ptr()
                assert_same_bits(got_a, want_a, what + " clamped")
                assert_same_bits(got_t, want_t, what + " target")
                assert (cbuf[:, d:] == POISON).all() and (tbuf[:, d:] == POISON).all(), what + ": wrote behind the last column"
                if fz is not None:
                    assert (got_t[:, fz.to(dev)] == 0).all()
    # what the NaN / inf actions become (torch.clamp): NaN stays, +-inf meet the bound
    want_a, _ = M.targets(a, 1.0, offset, scale)
    assert want_a.isnan().sum() == 1 and (want_a[~want_a.isnan()].abs() <= 1).all()


def test_kernel_allocates_and_clamps_in_place(dev):
    a, _, _, g = _inputs(5, 69, 9)
    offset, scale = _tables(69, g)
    want_a, want_t = M.targets(a, 1.0, offset, scale)
    ad = a.to(dev)
    got_a, got_t = ops.pd_targets(ad, scale.to(dev), clip=1.0, offset=offset.to(dev))
    assert got_a.is_contiguous() and got_a.data_ptr() != ad.data_ptr() and torch.equal(ad.cpu().nan_to_num(7.0), a.nan_to_num(7.0))     # the input is kept
    assert_same_bits(got_a, want_a, "clamped"), assert_same_bits(got_t, want_t, "target")
    got_a, got_t = ops.pd_targets(ad, scale.to(dev), clip=1.0, clamped=ad)                   # in place, offset absent = 0
    assert got_a.data_ptr() == ad.data_ptr()
    assert_same_bits(ad, want_a, "clamped in place"), assert_same_bits(got_t, M.targets(a, 1.0, torch.zeros(69), scale)[1], "target, no offset")


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
def test_kernel_16_byte_form_and_its_fall_back(dev, res):
    """D and every pitch a multiple of four floats, every base 16-byte aligned: the rows move as 16-byte accesses; a base off by one float must
    take the scalar form (a misaligned 16-byte access would fault or tear)."""
    n, d = 33, 72
    a, ref, sim, g = _inputs(n, d, 5)
    offset, scale = _tables(d, g)
    fz = torch.zeros(d, dtype=torch.bool)
    fz[0:3], fz[d - 3:d], fz[37] = True, True, True                              # bytes in every position of a 4-byte mask word
    want_a, want_t = M.targets(a, 1.0, offset, scale, fz, ref if res else None, sim if res else None)
    for shift in (0, 1):
        def place(t, fill=0.0):
            buf = torch.full((n * 76 + 4,), fill, dtype=torch.float32, device=dev)
            v = buf[shift:shift + n * 76].view(n, 76)[:, :d]
            v.copy_(t.to(dev))
            return buf, v
        (_, av), (_, rv), (_, sv) = place(a), place(ref), place(sim)
        cbuf, cv = place(torch.full((n, d), POISON), POISON)
        tbuf, tv = place(torch.full((n, d), POISON), POISON)
        assert av.data_ptr() % 16 == 4 * shift
        got_a, got_t = ops.pd_targets(av, scale.to(dev), clip=1.0, offset=offset.to(dev), freeze=fz.to(dev), ref_dof_pos=rv if res else None,
                                      sim_dof_pos=sv if res else None, clamped=cv, target=tv)
        assert_same_bits(got_a, want_a, f"shift {shift} clamped"), assert_same_bits(got_t, want_t, f"shift {shift} target")
        for buf in (cbuf, tbuf):
            rest = buf[shift:shift + n * 76].view(n, 76)[:, d:]
            assert (rest == POISON).all() and (buf[:shift] == POISON).all() and (buf[shift + n * 76:] == POISON).all()


def test_wrapper_rejects_what_the_kernel_cannot_take(dev):
    a = torch.zeros(4, 69, device=dev)
    s = torch.ones(69, device=dev)
    with pytest.raises(ValueError):
        ops.pd_targets(a.cpu(), s)
    with pytest.raises(ValueError, match="clip"):
        ops.pd_targets(a, s, clip=-1.0)
    with pytest.raises(ValueError, match="together"):
        ops.pd_targets(a, s, ref_dof_pos=a)
    with pytest.raises(ValueError, match="scale"):
        ops.pd_targets(a, s[:68])
    with pytest.raises(ValueError, match="target"):
        ops.pd_targets(a, s, target=torch.zeros(4, 68, device=dev))
    with pytest.raises(TypeError):
        ops.pd_targets(a, s, freeze=torch.zeros(69, device=dev))


# ------------------------------------------------------------------------------------------------------------------------------ env level
def _model_tables(nb, lims, robot, upright):
    mode = "none" if not robot.get("has_smpl_pd_offset") else ("upright" if upright else "not_upright")
    offset, scale = M.offset_scale(nb, lims[0], lims[1], bool(robot.get("bias_offset")), mode)
    return offset, scale, M.freeze_columns(nb, bool(robot.get("freeze_hand")), bool(robot.get("freeze_toe")))


ENV_CASES = [("smpl", {"bias_offset": True}, {}), ("smpl", {"has_smpl_pd_offset": True}, {}), ("smpl", {"freeze_toe": True}, {}),
             ("smpl", {"freeze_hand": True}, {}), ("smpl", {}, {}), ("smpl", {"freeze_toe": True, "freeze_hand": True}, {"res_action": True}),
             ("smplx", {"freeze_toe": True, "has_smpl_pd_offset": True}, {})]


@pytest.mark.parametrize("humanoid,robot,env_over", ENV_CASES, ids=lambda v: "+".join(sorted(v)) or "shipped" if isinstance(v, dict) else v)
def test_env_targets_equal_the_model_with_published_limits(dev, humanoid, robot, env_over):
    n, nb = 33, syn.skeleton(humanoid)["num_bodies"]
    lims = syn.synthetic_dof_limits(humanoid)
    env, _ = configs.make_env(n, 8, dev, seed=5, reference="motion_lib", humanoid=humanoid, env_overrides=env_over, robot_overrides=robot,
                              dof_limits=lims)
    task = env.task
    offset, scale, fz = _model_tables(nb, lims, robot, upright=humanoid == "smpl")
    assert_same_bits(task._pd_action_offset, offset, "offset table"), assert_same_bits(task._pd_action_scale, scale, "scale table")
    env.reset()
    g = torch.Generator().manual_seed(3)
    for _ in range(2):
        act = M.ACTION_SIGMA * torch.randn(n, 3 * (nb - 1), generator=g)
        res = bool(env_over.get("res_action"))
        ref, sim = (task._track["dof_pos"].cpu().clone(), task.sim.dof_pos.cpu().clone()) if res else (None, None)
        env.step(act.to(dev))
        want_a, want_t = M.targets(act, 1.0, offset, scale, fz, ref, sim)
        assert_same_bits(task.sim.pd_targets, want_t, "sim.pd_targets"), assert_same_bits(task.actions, want_a, "task.actions")
    if fz.any():
        assert (task.sim.pd_targets[:, fz.to(dev)] == 0).all()
    if not robot:
        assert not (task.sim.pd_targets.cpu() == act.clamp(-1, 1)).all()                      # the limits alone change the targets (scale)


def test_downstream_task_targets_equal_the_model(dev):
    from pulse_amd.env import humanoid_tasks as HT
    n = 33
    lims = syn.synthetic_dof_limits("smpl", seed=2)
    # has_upright_start is read from cfg.robot (humanoid.py:355): the shoulder offsets must be the non-upright ones
    robot = {"humanoid_type": "smpl", "freeze_toe": True, "bias_offset": True, "has_smpl_pd_offset": True, "has_upright_start": False}
    sim = HT.SyntheticTaskSim(n, 8, dev, seed=2, dof_limits=lims)
    task = HT.HumanoidSpeed({"env": {"episode_length": 1000}, "robot": robot}, sim, device=dev)
    from pulse_amd.env.humanoid_im import VecTaskPythonWrapper
    env = VecTaskPythonWrapper(task, rl_device=dev)
    env.reset()
    offset, scale, fz = _model_tables(24, lims, robot, upright=False)
    assert task._has_upright_start is False and np.count_nonzero(offset.numpy() == np.float32(-np.pi / 6)) == 1
    assert_same_bits(task._pd_action_offset, offset, "offset table"), assert_same_bits(task._pd_action_scale, scale, "scale table")
    act = M.ACTION_SIGMA * torch.randn(n, 69, generator=torch.Generator().manual_seed(1))
    env.step(act.to(dev))
    want_a, want_t = M.targets(act, 1.0, offset, scale, fz)
    assert_same_bits(sim.pd_targets, want_t, "sim.pd_targets"), assert_same_bits(task.actions, want_a, "task.actions")
    # no limits, no switches: the targets are the clamped action
    sim2 = HT.SyntheticTaskSim(n, 8, dev, seed=2)
    env2 = VecTaskPythonWrapper(HT.HumanoidSpeed({"env": {"episode_length": 1000}}, sim2, device=dev), rl_device=dev)
    env2.reset()
    env2.step(act.to(dev))
    assert torch.equal(sim2.pd_targets.cpu(), act.clamp(-1, 1))


class _AtenLog(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(func.__name__)
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize("humanoid,reference", [("smpl", "motion_lib"), ("smpl", "recorded"), ("smplx", "motion_lib")])
def test_default_targets_are_the_clamped_action_in_one_launch(dev, monkeypatch, humanoid, reference):
    """No published limits, no robot switches (every config that existed before the stage): targets = 0 + 1 * clamp(actions), and the stage is one
    pulse_pd_targets launch -- no torch clamp in the wrapper, no addcmul in the task."""
    n, d = 33, syn.skeleton(humanoid)["num_dof"]
    env, _ = configs.make_env(n, 8, dev, seed=5, reference=reference, humanoid=humanoid)
    env.reset()
    launches = []
    real = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, *a, **k: (launches.append(name), real(name, *a, **k))[1])
    act = (M.ACTION_SIGMA * torch.randn(n, d, generator=torch.Generator().manual_seed(2))).to(dev)
    with _AtenLog() as log:
        env.step(act)
    want = act.clamp(-1, 1)
    assert torch.equal(env.task.sim.pd_targets, want) and torch.equal(env.task.actions, want)
    assert_same_bits(env.task.sim.pd_targets, torch.addcmul(torch.zeros(d, device=dev), torch.ones(d, device=dev), want), "targets")
    assert launches.count("pulse_pd_targets") == 1
    assert not [nm for nm in log.names if nm.split(".")[0] in ("clamp", "addcmul", "clamp_", "minimum", "maximum")], log.names
    assert float((act.abs() > 1).float().mean()) > 0.2


def test_latent_env_keeps_the_wrapper_clamp_on_the_latent(dev):
    """The latent envs' step() takes z: the wrapper's clip bounds z, the decoded PD action is not clamped (as before the stage was fused)."""
    env, _ = configs.make_env(16, 4, dev, seed=5, env_kind="speed_z")
    assert env._task_clips is False and env.task._actuation.clip == float("inf")
    env.reset()
    z = 3.0 * torch.randn(16, 32, generator=torch.Generator().manual_seed(4)).to(dev)
    env.step(z)
    assert torch.equal(env.task.action_z, z.clamp(-1, 1))
    assert torch.equal(env.task.sim.pd_targets, env.task.actions)
    env_im, _ = configs.make_env(16, 4, dev, seed=5, reference="motion_lib")
    assert env_im._task_clips is True and env_im.task._actuation.clip == 1.0
