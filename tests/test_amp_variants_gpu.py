"""GPU: the AMP frame kernels (amp_obs.hip) in their configured variants -- discriminator shape / limb rows, non-upright root, amp_obs_v 2,
history mode for any frame width -- against tests/golden/env_amp_variants.npz (the reference's own functions) and tests/amp_frame_model.py
(the restatement tests/test_amp_variants_cpu.py holds to that fixture and to HumanoidAMP's method bodies bit for bit), from the kernel up
to the env and the agent.  Tolerance: atol = rtol = 1e-5 (``close``, as tests/test_env_kernels_gpu.py); copied columns and bit claims exact."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import amp_frame_model as M
from oracle.motion_oracle import OracleMotionLib
from pulse_amd import configs, ops, synthetic as syn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(a, b, atol=1e-5, rtol=1e-5, msg=""):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    np.testing.assert_allclose(a, b, atol=atol, rtol=rtol, equal_nan=True, err_msg=msg)


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_golden_amp_variants", os.path.join(ROOT, "tools", "gen_golden_amp_variants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture(gen):
    z, d = gen.load(), gen.inputs()
    for k, v in gen.input_sums(d).items():
        assert v.item() == z[k].item(), f"{k}: the input recipe draws other numbers than the committed fixture was generated from"
    return z, d


def spec_kwargs(gen, d, spec, dev):
    """The keyword arguments of ops.build_amp_observations_smpl for a fixture variant (inputs ``d`` already on ``dev``)."""
    return {"joint_ids": torch.tensor(gen.JOINTS19, dtype=torch.int32, device=dev) if spec["subset"] else None, "root_height_obs": spec["height"],
            "upright": spec["upright"], "version": spec["version"], "shape_params": d["shapes"][:, :-6] if spec["shape"] else None,
            "limb_weights": d["limbs"] if spec["limb"] else None}


def model_frame(gen, d, spec):
    return M.frame_from_records(d["rb"], d["dof_pos"], d["dof_vel"], gen.KEY, d["shapes"][:, :-6] if spec["shape"] else None,
                                d["limbs"] if spec["limb"] else None, dof_subset=torch.tensor(gen.SUBSET) if spec["subset"] else None,
                                root_height_obs=spec["height"], upright=spec["upright"], version=spec["version"])


def to_dev(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ 1. kernel against fixture
def test_kernel_matches_every_fixture_variant(gen, fixture, dev):
    z, d = fixture
    dd = to_dev(d, dev)
    key = torch.tensor(gen.KEY, device=dev)
    n = gen.N
    ids = torch.tensor([36, 0, 5, 17, 4, 3, 22], device=dev)
    mask = torch.zeros(n, dtype=torch.bool, device=dev)
    mask[[1, 2, 3, 8, 35, 36]] = True
    for name, spec in gen.VARIANTS.items():
        kw = spec_kwargs(gen, dd, spec, dev)
        want = z[name]
        w = want.shape[1]
        got = ops.build_amp_observations_smpl(dd["rb"], dd["dof_pos"], dd["dof_vel"], key, **kw)
        assert got.shape == want.shape, name
        close(got, want, msg=name)
        c = gen.columns(spec)
        assert np.array_equal(got[:, c["rows"]].cpu().numpy(), want[:, c["rows"]]), f"{name}: copied shape / limb columns"
        # an output pitch larger than W, an env_ids subset and an env_mask subset: everything else stays untouched
        for sub in ({"env_ids": ids}, {"env_mask": mask}, {"env_ids": ids, "env_mask": mask}):
            out = torch.full((n, w + 5), float("nan"), device=dev)
            ops.build_amp_observations_smpl(dd["rb"], dd["dof_pos"], dd["dof_vel"], key, out=out, **sub, **kw)
            sel = torch.zeros(n, dtype=torch.bool, device=dev)
            sel[ids] = True
            if "env_ids" not in sub:
                sel[:] = True
            if "env_mask" in sub:
                sel &= mask
            assert sel.any() and not sel.all()
            want_out = np.full((n, w + 5), np.nan, dtype=np.float32)
            want_out[sel.cpu().numpy(), :w] = want[sel.cpu().numpy()]
            close(out, want_out, msg=f"{name} {sorted(sub)}")


@pytest.mark.parametrize("n", [1, 4, 5])
def test_kernel_matches_restatement_at_block_edges(gen, dev, n):
    """One block of 4 envs, its edge, one past it."""
    d = gen.inputs(n, seed=gen.SEED + n)
    dd = to_dev(d, dev)
    key = torch.tensor(gen.KEY, device=dev)
    for name, spec in gen.VARIANTS.items():
        got = ops.build_amp_observations_smpl(dd["rb"], dd["dof_pos"], dd["dof_vel"], key, **spec_kwargs(gen, dd, spec, dev))
        close(got, model_frame(gen, d, spec), msg=f"{name} n={n}")


def test_argument_checks(gen, dev):
    d = to_dev(gen.inputs(5), dev)
    key = torch.tensor(gen.KEY, device=dev)
    run = lambda **kw: ops.build_amp_observations_smpl(d["rb"], d["dof_pos"], d["dof_vel"], key, **kw)
    with pytest.raises(ValueError, match="version"):
        run(version=3)
    with pytest.raises(TypeError, match="shape_params"):
        run(shape_params=d["shapes"][:4, :11])                       # one row per env
    with pytest.raises(TypeError, match="limb_weights"):
        run(limb_weights=d["limbs"].double())
    with pytest.raises(TypeError, match="shape_params"):
        run(shape_params=d["shapes"].cpu()[:, :11])
    with pytest.raises(TypeError, match="limb_weights"):
        run(limb_weights=d["limbs"].t().contiguous().t())            # column stride != 1


# ------------------------------------------------------------------------------------------------ 2. history mode for any W
@pytest.mark.parametrize("S", [2, 10])
@pytest.mark.parametrize("case", ["W207_unaligned", "W208_aligned", "W208_unaligned_sink"])
def test_history_mode_equals_op_by_op_for_any_width(gen, dev, S, case):
    """Five steps over a random stream of states: shift + current frame (+ copy into window_out) in one launch against the same three
    operations done with torch on the device (bit-identical) and against the restatement (1e-5)."""
    n = 9                                                            # three blocks, the last with one env
    if case == "W207_unaligned":
        spec, pad = dict(version=1, upright=False, subset=True, height=True, shape=True, limb=False), 5
    elif case == "W208_aligned":
        spec, pad = dict(version=2, upright=True, subset=True, height=True, shape=False, limb=False), 4
    else:
        spec, pad = dict(version=2, upright=False, subset=True, height=True, shape=False, limb=False), 3
    W = gen.columns(spec)["width"]
    assert W == (207 if case == "W207_unaligned" else 208)
    key = torch.tensor(gen.KEY, device=dev)
    g = torch.Generator().manual_seed(100 + S)
    init = torch.randn(n, S, W, generator=g)
    for with_sink in (False, True):
        fused, plain = init.to(dev).clone(), init.to(dev).clone()
        model = init.clone()
        sink = torch.full((n, S * W + pad), float("nan"), device=dev) if with_sink else None
        assert ((S * W + pad) % 4 == 0) == (case == "W208_aligned")                      # only that case takes the float4 copies
        for step in range(5):
            d = gen.inputs(n, seed=500 + 10 * S + step)
            dd = to_dev(d, dev)
            kw = spec_kwargs(gen, dd, spec, dev)
            ops.build_amp_observations_smpl(dd["rb"], dd["dof_pos"], dd["dof_vel"], key, out=fused[:, 0], hist_steps=S, window_out=sink, **kw)
            plain[:, 1:] = plain[:, 0:S - 1].clone()                                     # _update_hist_amp_obs
            ops.build_amp_observations_smpl(dd["rb"], dd["dof_pos"], dd["dof_vel"], key, out=plain[:, 0], **kw)      # _compute_amp_observations
            model[:, 1:] = model[:, 0:S - 1].clone()
            model[:, 0] = model_frame(gen, d, spec)
            assert torch.equal(fused, plain), f"{case} S={S} step {step}: window differs from the op-by-op sequence"
            close(fused, model, msg=f"{case} S={S} step {step}")
            if with_sink:
                assert torch.equal(sink[:, :S * W], plain.view(n, -1)), f"{case} S={S} step {step}: window_out"
                assert torch.isnan(sink[:, S * W:]).all()


# ------------------------------------------------------------------------------------------------ 3. history init from the motion
def test_amp_hist_init_with_motion_rows_non_upright_v2(gen, dev):
    from pulse_amd.env.motion_lib import MotionLib
    n, S, dt, m = 9, 10, 2.0 / 60.0, 6
    tabs = M.non_upright_tables(syn.synthetic_motion_library(syn.make_generator(77), m, 20, 40, shape_rows=True))
    lib = MotionLib.from_tables(tabs, dev)
    ids = torch.tensor([0, 5, 2, 2, 1, 4, 3, 5, 0])
    starts = torch.tensor([0.0, 0.1, 0.4, 0.05, 0.6, 0.2, 0.3, 0.5, 0.15])            # 9 history frames reach back 0.3 s: most envs cross the clip start
    assert (starts - dt * (S - 1) < 0).sum() >= 5 and (starts - dt * (S - 1) > 0).sum() >= 2
    mask = torch.tensor([1, 1, 0, 1, 1, 0, 1, 0, 1], dtype=torch.bool)
    spec = dict(version=2, upright=False, subset=True, height=True, shape=True, limb=True)
    W = gen.columns(spec)["width"]
    assert W == 208 + 21
    hist = torch.full((n, S, W), float("nan"), device=dev)
    ops.amp_hist_init(lib, ids.to(dev), starts.to(dev), dt, mask.to(dev), hist, torch.tensor(gen.KEY, device=dev),
                      joint_ids=torch.tensor(gen.JOINTS19, dtype=torch.int32, device=dev), upright=False, version=2,
                      shape_params=lib.motion_bodies[:, :-6], limb_weights=lib.motion_limb_weights)
    twin = M.AmpWindow(OracleMotionLib(tabs), ids, S, dt, gen.KEY, dof_subset=torch.tensor(gen.SUBSET), motion_bodies=tabs["motion_bodies"],
                       motion_limb_weights=tabs["motion_limb_weights"], has_shape_obs_disc=True, has_limb_weight_obs_disc=True, upright=False, version=2)
    k = S - 1
    times = (starts.unsqueeze(-1) + (-dt * (torch.arange(0, k) + 1))).view(-1)
    want = torch.full((n, S, W), float("nan"))
    want[:, 1:] = twin.motion_frames(ids.repeat_interleave(k), times).view(n, k, W)
    want[~mask] = float("nan")                                                        # masked-out rows and slot 0 untouched
    close(hist, want)
    got = hist.cpu()
    assert torch.equal(got[mask][:, 1:, -21:-10], tabs["motion_bodies"][ids[mask], :11][:, None].expand(-1, k, -1))       # the MOTION's rows, copied
    assert torch.equal(got[mask][:, 1:, -10:], tabs["motion_limb_weights"][ids[mask]][:, None].expand(-1, k, -1))
    with pytest.raises(TypeError, match="shape_params"):                              # one row per motion, not per env
        ops.amp_hist_init(lib, ids.to(dev), starts.to(dev), dt, mask.to(dev), hist, torch.tensor(gen.KEY, device=dev),
                          joint_ids=torch.tensor(gen.JOINTS19, dtype=torch.int32, device=dev), upright=False, version=2,
                          shape_params=torch.zeros(n, 11, device=dev), limb_weights=lib.motion_limb_weights)


# ------------------------------------------------------------------------------------------------ 4. env level
ENV_DICTS = {
    # the AMP-relevant part of phc/data/cfg/env/phc_shape_pnn_iccv.yaml
    "phc_shape_pnn_iccv": {"has_shape_obs": True, "has_shape_obs_disc": True, "has_dof_subset": True, "has_upright_start": True, "numAMPObsSteps": 10},
    "noup_v2_limb": {"has_upright_start": False, "amp_obs_v": 2, "has_weight_obs_disc": True, "has_dof_subset": True, "numAMPObsSteps": 10},
}


@pytest.mark.parametrize("which", sorted(ENV_DICTS))
def test_env_windows_and_demo_match_restatement(dev, monkeypatch, which):
    """16 envs on the motion-library reference, eight steps with a reset in the middle: extras['amp_obs'], the window after resets and
    fetch_amp_obs_demo(32) against the restatement driven with the same states and the same sampled ids / times; PULSE_AMP_FUSED=0 gives the
    same bits."""
    from pulse_amd.env.humanoid_im import HumanoidIm, VecTaskPythonWrapper
    from pulse_amd.env.motion_lib import MotionLib
    from pulse_amd.env.sim import KinematicSim
    n, seed, over = 16, 31, ENV_DICTS[which]
    shape_disc, limb_disc = bool(over.get("has_shape_obs_disc")), bool(over.get("has_weight_obs_disc"))
    version, upright = int(over.get("amp_obs_v", 1)), bool(over["has_upright_start"])
    W = 196 + 12 * (version == 2) + 11 * shape_disc + 10 * limb_disc

    def run(fused, check):
        monkeypatch.setenv("PULSE_AMP_FUSED", "1" if fused else "0")
        tabs = syn.synthetic_motion_library(syn.make_generator(seed + 5, 0), n, shape_rows=True)            # make_env's library
        if upright:
            env, _ = configs.make_env(n, 12, dev, seed=seed, env_kind="amp", reference="motion_lib", env_overrides=over)
        else:                                 # the same env over the motions of a non-upright humanoid (M.non_upright_tables says why)
            tabs = M.non_upright_tables(tabs)
            task = HumanoidIm({"env": dict(configs.ENV_IM, enable_amp_obs=True, **over)}, KinematicSim(n, 13, dev, seed=seed, rank=0, humanoid="smpl"),
                              MotionLib.from_tables(tabs, dev), device=dev)
            env = VecTaskPythonWrapper(task, rl_device=dev)
        task, sim = env.task, env.task.sim
        assert task._amp_fused == fused and task._num_amp_obs_per_step == W and task.get_num_amp_obs() == 10 * W
        assert env.get_env_info()["amp_observation_space"].shape == (10 * W,)
        assert torch.equal(task._motion_lib.motion_bodies.cpu(), tabs["motion_bodies"])
        twin = M.AmpWindow(OracleMotionLib(tabs), task._sampled_motion_ids.cpu(), 10, task.dt, task._key_body_ids.cpu().long(),
                           dof_subset=torch.tensor([3 * int(j) + k for j in task._amp_joint_ids.cpu() for k in range(3)]),
                           shapes=task.humanoid_shapes.cpu(), limbs=task.humanoid_limb_and_weights.cpu(), motion_bodies=tabs["motion_bodies"],
                           motion_limb_weights=tabs["motion_limb_weights"], has_shape_obs_disc=shape_disc, has_limb_weight_obs_disc=limb_disc,
                           upright=upright, version=version)
        state = lambda: (sim.rigid_body_state.cpu().clone(), sim.dof_pos.cpu().clone(), sim.dof_vel.cpu().clone())
        out = []
        env.reset()
        if check:
            twin.reset(torch.arange(n), *state(), task._motion_start_times.cpu(), from_motion=True)
            close(task._amp_obs_buf, twin.buf, msg="window after the first reset")
        out.append(task._amp_obs_buf.clone())
        for step in range(8):
            obs, rew, done, info = env.step(torch.zeros(n, 69, device=dev))
            out.append(info["amp_obs"].clone())
            if check:
                close(info["amp_obs"], twin.step(*state()), msg=f"amp_obs step {step}")
            ids = torch.nonzero(done).flatten()
            if step == 3:                                                          # the reset in the middle, whatever terminated
                ids = torch.unique(torch.cat([ids, torch.tensor([1, 5, 6, 15], device=dev)]))
            env.reset(ids)
            if check:
                twin.reset(ids.cpu(), *state(), task._motion_start_times.cpu(), from_motion=True)
                close(task._amp_obs_buf, twin.buf, msg=f"window after reset {step}")
            out.append(task._amp_obs_buf.clone())
        gstate = task._clock_gen.get_state()
        demo = env.fetch_amp_obs_demo(32)
        assert demo.shape == (32, 10 * W)
        out.append(demo.clone())
        if check:
            task._clock_gen.set_state(gstate)                                      # the same draws again: the sampled ids / times
            mids = task._motion_lib.sample_motions(32, generator=task._clock_gen)
            t0 = task._motion_lib.sample_time_interval(mids, generator=task._clock_gen)
            close(demo, twin.demo(mids.cpu(), t0.cpu()), msg="demo windows")
            rows = demo.view(32, 10, W)[:, :, 196 + 12 * (version == 2):].cpu()    # the MOTION's rows in every frame of a demo window
            want_rows = torch.cat(([tabs["motion_bodies"][mids.cpu(), :11]] if shape_disc else []) +
                                  ([tabs["motion_limb_weights"][mids.cpu()]] if limb_disc else []), dim=-1)
            assert torch.equal(rows, want_rows[:, None].expand(-1, 10, -1))
        return out

    a, b = run(True, True), run(False, False)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x.reshape(x.shape[0], -1), y.reshape(y.shape[0], -1)), f"output {i}: the fused and the op-by-op path differ"


def test_env_option_errors(dev):
    with pytest.raises(NotImplementedError, match="amp_obs_v 2 with has_shape_obs_disc"):
        configs.make_env(8, 4, dev, env_kind="amp", reference="motion_lib", env_overrides={"amp_obs_v": 2, "has_shape_obs_disc": True})
    with pytest.raises(ValueError, match="amp_obs_v = 3"):
        configs.make_env(8, 4, dev, env_kind="amp", env_overrides={"amp_obs_v": 3})
    from pulse_amd.env.humanoid_im import HumanoidIm
    from pulse_amd.env.motion_lib import MotionLib
    from pulse_amd.env.sim import KinematicSim
    lib = MotionLib.from_tables(syn.synthetic_motion_library(syn.make_generator(3), 8), dev)       # no shape rows
    with pytest.raises(ValueError, match="has_shape_obs_disc: the motion library carries no motion_bodies"):
        HumanoidIm({"env": dict(configs.ENV_IM, enable_amp_obs=True, has_shape_obs_disc=True)}, KinematicSim(8, 5, dev, seed=1, rank=0, humanoid="smpl"), lib, device=dev)


# ------------------------------------------------------------------------------------------------ 5. agent
def test_agent_trains_on_the_shape_aware_window_and_restores(dev):
    torch.manual_seed(3)
    over = ENV_DICTS["phc_shape_pnn_iccv"]
    ag, _ = configs.make_agent("cfg5_small", device=dev, seed=7, env_overrides=over)
    assert ag.vec_env.env.task._num_amp_obs_per_step == 207 and ag._amp_dim == 2070
    assert any(v.dim() == 2 and v.shape[1] == 2070 for v in ag.disc.state_dict().values()), "no discriminator layer takes 2070 inputs"
    disc0 = ag.disc.flat.clone()
    info = ag.train_epoch()
    for k in ("disc_loss", "disc_grad_penalty", "disc_agent_acc", "disc_demo_acc", "actor_loss", "critic_loss", "grad_norm"):
        v = torch.stack([torch.as_tensor(t, device=dev).float() for t in info[k]])
        assert torch.isfinite(v).all(), k
    assert torch.isfinite(info["disc_rewards"]).all() and not torch.equal(disc0, ag.disc.flat)
    # the shape columns reached the experience buffer: frame 0 of every recorded window ends in the env's shape row
    amp = ag.experience_buffer.flat("amp_obs")[:, :2070].view(ag.num_actors, ag.horizon_length, 10, 207)
    task = ag.vec_env.env.task
    assert torch.equal(amp[:, :, 0, 196:], task.humanoid_shapes[:, None, :11].expand(-1, ag.horizon_length, -1))

    def logits(agent, x):
        xs = torch.zeros(x.shape[0], agent._amp_pitch, device=dev)
        agent._amp_input_mean_std.forward(x, out=xs, out_cols=agent._amp_pitch, update=False)
        return agent.disc.eval_disc(xs).clone()

    x = torch.randn(64, ag._amp_pitch, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    ag.set_eval()
    la = logits(ag, x)
    other, _ = configs.make_agent("cfg5_small", device=dev, seed=11, env_overrides=over)
    other.set_eval()
    assert la.shape == (64, 1) and torch.isfinite(la).all() and not torch.equal(la, logits(other, x))
    other.set_full_state_weights(ag.get_full_state_weights())
    assert torch.equal(la, logits(other, x)), "the restored agent does not reproduce the discriminator's logits"


# ------------------------------------------------------------------------------------------------ 6. the path that exists
def test_default_arguments_are_todays_frame(golden, dev):
    g = golden("env_amp.npz")
    rb, dp, dv, key = g.t("rb", dev), g.t("dof_pos", dev), g.t("dof_vel", dev), g.t("key_body_ids", dev)
    j19 = g.t("joints19", dev).int()
    explicit = {"upright": True, "version": 1, "shape_params": None, "limb_weights": None}
    for kw, name in (({}, "amp_obs_full"), ({"joint_ids": j19, "root_height_obs": False}, "amp_obs_subset19_noheight"),
                     ({"local_root_obs": False}, "amp_obs_global_root")):
        a = ops.build_amp_observations_smpl(rb, dp, dv, key, **kw)
        close(a, g.np(name), msg=name)
        assert torch.equal(a, ops.build_amp_observations_smpl(rb, dp, dv, key, **kw, **explicit)), name
    assert ops.amp_obs_width(23, 4) == 232 and ops.amp_obs_width(19, 4, False) == 195
