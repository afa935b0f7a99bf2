"""CPU: the yardsticks pulse_keypoint_push is held to, and everything of the keypoint stream that needs no device.

  * ``kernels.keypoint_taps`` against scipy's own mirror-mode impulse responses;
  * tests/keypoint_stream_model.py in float64 against tests/golden/keypoint_stream.npz -- the body of the reference's _compute_task_obs_demo run
    step by step (tools/gen_golden_keypoint_stream.py).  The reference rounds p_f + trans_f to float32 and then forms a 3-term product in
    float32: positions agree to 4 * 2^-23 * max |pos|, velocities (a difference of two such values, times 30) to 60 times that;
  * the fixture's observation is compute_imitation_observations_v7 fed oracle.env_oracle.zero_out_far_refs of the fixture's pos / vel: the
    demo's masking is the masking pulse_im_step already has.  Bit for bit with the reference's own function where the reference checkout is
    present; elsewhere the oracle's restatement stands in, to the cross-host floor of oracle/refrecord.py;
  * the fixture's conditions (regimes per step, margins), per-env clear on the model, rejections by name, the config, the entry point's struct."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden_keypoint_stream as GK  # noqa: E402
import keypoint_stream_model as KM  # noqa: E402
from oracle import env_oracle as E  # noqa: E402
from oracle import refload, refrecord  # noqa: E402
from pulse_amd import _lib, configs, kernels  # noqa: E402
from pulse_amd import synthetic as syn  # noqa: E402
from pulse_amd.env import humanoid_im_demo as HD  # noqa: E402
from pulse_amd.env.keypoint_stream import KeypointStream  # noqa: E402

INVALID = -1


@pytest.fixture(scope="module")
def fx():
    return GK.load()


# ------------------------------------------------------------------------------------------------------------------ the tap table
def test_taps_are_scipys_mirror_impulse_responses():
    from scipy.ndimage import gaussian_filter1d
    taps = kernels.keypoint_taps()
    assert taps.shape == (3, 30, 30) and taps.dtype == np.float64
    worst = 0.0
    for k, sigma in enumerate((10.0, 5.0, 2.0)):
        for length in range(1, 31):
            want = np.array([gaussian_filter1d(np.eye(length)[i], sigma, mode="mirror")[-1] for i in range(length)])
            row = taps[k, length - 1]
            worst = max(worst, float(np.abs(row[:length] - want).max()))
            assert not row[length:].any()
            assert abs(row.sum() - 1.0) <= 1e-14, (sigma, length)
        assert np.array_equal(taps[k, 0, :1], [1.0])
    print(f"taps vs scipy: max difference {worst:.3e}")
    assert worst <= 1e-14
    assert kernels.keypoint_taps((2.0,), history=4).shape == (1, 4, 4)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="history"):
            kernels.keypoint_taps(history=bad)


# ------------------------------------------------------------------------------------------------------------------ model vs reference
@pytest.mark.parametrize("name", sorted(GK.STREAMS))
def test_model_reproduces_the_reference_body(fx, name):
    frames, history = GK.STREAMS[name]
    assert int(fx[f"history_{name}"]) == history and fx[f"j3d_{name}"].shape == (frames, GK.N, GK.J, 3) and fx[f"j3d_{name}"].dtype == np.float32
    pos, vel = KM.run(fx[f"j3d_{name}"], history, np.float64)
    assert np.array_equal(pos, fx[f"pos64_{name}"]) or float(np.abs(pos - fx[f"pos64_{name}"]).max()) <= 1e-13       # the stored fp64 run is this model's
    bound_pos = 4 * 2.0 ** -23 * float(np.abs(fx[f"pos_{name}"]).max())
    gap_pos = float(np.abs(pos - fx[f"pos_{name}"]).max())
    gap_vel = float(np.abs(vel - fx[f"vel_{name}"]).max())
    print(f"stream {name}: model64 vs reference body: pos {gap_pos:.3e} (bound {bound_pos:.3e}), vel {gap_vel:.3e} (bound {60 * bound_pos:.3e})")
    assert gap_pos <= bound_pos and gap_vel <= 60 * bound_pos
    # the first velocity is pos / dt: prev_pos starts at zero, the reference's behaviour
    assert np.array_equal(fx[f"vel_{name}"][0], fx[f"pos_{name}"][0] / np.float32(1 / 30))


@pytest.mark.parametrize("name", sorted(GK.STREAMS))
def test_fixture_observation_is_the_masking_the_step_kernel_has(fx, name):
    live = refrecord.live()
    v7 = refload.env_functions()["compute_imitation_observations_v7"] if live else None
    close, far = float(fx["close_distance"]), float(fx["far_distance"])
    assert close == 0.5
    for t in range(GK.STREAMS[name][0]):
        bp, br, bv, ba = E.split_rb(torch.from_numpy(fx["rb"][t]))
        ref_pos, ref_vel = torch.from_numpy(fx[f"pos_{name}"][t]), torch.from_numpy(fx[f"vel_{name}"][t])
        rp, _, rv, _, dist = E.zero_out_far_refs(7, bp[:, 0], bp, br, bv, ba, ref_pos, br, ref_vel, ba, close, far)
        want = torch.from_numpy(fx[f"obs_{name}"][t])
        if live:
            assert torch.equal(v7(bp[:, 0], br[:, 0], bp, bv, rp, rv, 1, True), want), (name, t)
        else:
            assert refrecord.close_across_hosts(E.im_obs_v7(bp[:, 0], br[:, 0], bp, bv, rp, rv, 1), want), (name, t)
        assert np.allclose(dist.numpy(), fx[f"dist_{name}"][t], atol=1e-5)


def test_fixture_holds_the_cases(fx):
    for name, (frames, history) in GK.STREAMS.items():
        d = fx[f"dist_{name}"]
        assert d.shape == (frames, 5)
        assert (np.abs(d - 0.5) > 1e-3).all() and (np.abs(d - float(fx["far_distance"])) > 1e-3).all()
        near, far = d < 0.5, d > float(fx["far_distance"])
        assert near.any(1).all() and far.any(1).all() and (~near & ~far).any(1).all()          # every step: all three masking regimes
        assert frames > history                                                               # wrapped pushes
    assert float(fx["err_pos"]) > 0 and float(fx["err_vel"]) > 0
    assert np.array_equal(fx["frame"], kernels.keypoint_frame("y_up").astype(np.float32))
    assert np.array_equal(fx["mean_limb_lengths"], np.array(kernels.KEYPOINT_MEAN_LIMB_LENGTHS, dtype=np.float32))
    assert np.array_equal(kernels.keypoint_frame("sim"), np.eye(3))


@pytest.mark.skipif(not refload.available(), reason="reference checkout not present: the fixture stands in for it")
def test_generator_reproduces_the_fixture(fx):
    live = GK.generate(verbose=False)
    assert set(live) == set(fx)
    for k in sorted(fx):
        assert np.array_equal(live[k], fx[k]), k


# ------------------------------------------------------------------------------------------------------------------ per-env counts
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_model_clear_is_a_fresh_stream_for_those_envs(fx, dtype):
    j3d, history = fx["j3d_A"], 30
    m = KM.StreamModel(5, history=history, dtype=dtype)
    plain = KM.StreamModel(5, history=history, dtype=dtype)
    fresh = KM.StreamModel(5, history=history, dtype=dtype)
    cleared = np.array([False, True, False, True, False])
    for t in range(20):
        if t == 12:
            m.clear(cleared)
        m.push(j3d[t])
        plain.push(j3d[t])
        if t >= 12:
            fresh.push(j3d[t])
            assert np.array_equal(m.pos[cleared], fresh.pos[cleared]) and np.array_equal(m.vel[cleared], fresh.vel[cleared])
            assert m.count[cleared].tolist() == [t - 11, t - 11]
        assert np.array_equal(m.pos[~cleared], plain.pos[~cleared]) and np.array_equal(m.vel[~cleared], plain.vel[~cleared])
    assert m.count.tolist() == [20, 8, 20, 8, 20]
    # a masked push leaves the env alone
    before = m.state()
    m.push(j3d[20], env_mask=[True, True, False, True, True])
    after = m.state()
    for k in before:
        assert np.array_equal(before[k][2], after[k][2]), k
    assert after["count"].tolist() == [21, 9, 20, 9, 21]


def test_coincident_keypoints_give_nan_as_the_reference_does():
    m = KM.StreamModel(2, history=4)
    frame = np.random.default_rng(0).standard_normal((2, 24, 3))
    frame[1] = frame[1, :1]                                       # env 1: every joint at one point -> scale 0 -> 0 / 0
    pos, _ = m.push(frame)
    assert np.isfinite(pos[0]).all() and np.isnan(pos[1]).all()


# ------------------------------------------------------------------------------------------------------------------ rejections by name
def _cfg(**env):
    return {"env": dict(configs.ENV_MCP_DEMO, **env), "robot": configs.robot_config("smpl")}


def test_rejections_need_no_device():
    with pytest.raises(NotImplementedError, match="obs_v 6 raises NotImplementedError in the reference itself"):
        HD.HumanoidImMCPDemo(_cfg(obs_v=6), sim=None)
    with pytest.raises(NotImplementedError, match="obs_v 6"):
        HD.HumanoidImDemo({"env": dict(configs.ENV_IM_DEMO, obs_v=6)}, sim=None)
    with pytest.raises(NotImplementedError, match="obs_v 9"):
        HD.check_demo_options(_cfg(obs_v=9))
    with pytest.raises(NotImplementedError, match="fut_tracks"):
        HD.HumanoidImMCPDemo(_cfg(fut_tracks=True), sim=None)
    with pytest.raises(NotImplementedError, match="enable_amp_obs"):
        HD.HumanoidImMCPDemo(_cfg(enable_amp_obs=True), sim=None)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match="history"):
            KeypointStream(5, "cpu", history=bad)
        with pytest.raises(ValueError, match="history"):
            HD.HumanoidImMCPDemo(_cfg(), sim=None, history=bad)
    with pytest.raises(ValueError, match="'y_up' or 'sim'"):
        KeypointStream(5, "cpu", frame="z_up")
    HD.check_demo_options(_cfg())                                  # the shipped demo config passes
    assert HD._demo_cfg(_cfg(zero_out_far_train=True))["env"]["zero_out_far_train"] is False


def test_a_bad_frame_is_refused_before_the_launch():
    s = KeypointStream(5, "cpu")                                  # host buffers: nothing here can launch
    good = torch.zeros(5, 24, 3)
    for bad, what in ((torch.zeros(5, 23, 3), "shape"), (torch.zeros(4, 24, 3), "shape"), (good.double(), "float32"),
                      (torch.zeros(5, 24, 6)[:, :, ::2], "unit inner stride"), (torch.zeros(5, 24, 3, device="meta"), "must live on"),
                      (good.numpy(), "torch.Tensor")):
        with pytest.raises(ValueError, match=what):
            s.push(bad)
    with pytest.raises(ValueError, match="env_mask"):
        s.push(good, env_mask=torch.ones(4, dtype=torch.bool))
    with pytest.raises(TypeError, match="CUDA tensor"):
        s.push(good)                                              # a stream on the host has no kernel to run: pulse_amd has no CPU path
    assert s.pushes == 0 and not s.count.any()
    with pytest.raises(NotImplementedError, match="KeypointStream.now"):
        s.now()
    with pytest.raises(NotImplementedError, match="sample_demo_states"):
        s.sample_demo_states(3)
    assert s.next() is s.next_after_reset() and s.next()["pos"] is s.pos and float(s._motion_lengths.min()) >= 1e8
    s.direct(torch.ones(1, 24, 3), torch.full((5, 24, 3), 2.0))
    assert (s.pos == 1).all() and (s.vel == 2).all()
    s.count[:] = 3
    s.prev_pos[:] = 1
    s.clear(torch.tensor([True, False, True, False, False]))
    assert s.count.tolist() == [0, 3, 0, 3, 3] and s.prev_pos[:, 0, 0].tolist() == [0, 1, 0, 1, 1]


def test_demo_configs():
    cfg, n = configs.agent_config("mcp_demo_small")
    assert n == 64 and cfg["_env_kind"] == "mcp_demo" and cfg["network"]["name"] == "amp_mcp"
    cfg, n = configs.agent_config("im_demo_small")
    assert n == 64 and cfg["_env_kind"] == "im_demo"
    assert configs.ENV_MCP_DEMO["obs_v"] == 7 and configs.ENV_IM_DEMO["obs_v"] == 7 and configs.ENV_MCP_DEMO["zero_out_far"]
    with pytest.raises(NotImplementedError, match="obs_v 6"):
        configs.make_env(8, 16, "cuda:0", env_kind="mcp_demo", env_overrides={"obs_v": 6})      # by name, before any device work


# ------------------------------------------------------------------------------------------------------------------ the entry point
def _args():
    a = _lib.KeypointPushArgs()
    a.num_envs, a.num_bodies, a.history, a.dt = 1, 24, 30, 1 / 30
    a.j3d_stride_n, a.j3d_stride_j = 72, 3
    a.joint_map[:24] = syn.smpl_joint_map()
    a.parent_indices[:24] = syn.SMPL_PARENTS
    for f in ("j3d", "taps", "root_ring", "body_ring", "count", "prev_pos", "pos", "vel"):
        setattr(a, f, 64)                                         # never dereferenced: every case below fails a check first
    return a


def test_struct_layout_and_launcher_checks():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.KeypointPushArgs) == lib.pulse_sizeof_keypoint_push_args()
    assert lib.pulse_keypoint_push(ctypes.byref(_lib.KeypointPushArgs()), None) == 0          # zero envs: nothing to do
    cases = [(lambda a: setattr(a, "num_bodies", 32), "num_bodies 32 not in"), (lambda a: setattr(a, "num_bodies", 5), "num_bodies 5 not in"),
             (lambda a: setattr(a, "history", 0), "history 0 not in"), (lambda a: setattr(a, "history", 65), "history 65 not in"),
             (lambda a: setattr(a, "dt", 0.0), "dt 0 must be positive"), (lambda a: setattr(a, "j3d", None), "null j3d"),
             (lambda a: setattr(a, "j3d_stride_j", 2), "at least 3 floats between joints"), (lambda a: setattr(a, "taps", None), "null taps"),
             (lambda a: setattr(a, "count", None), "null state"), (lambda a: setattr(a, "vel", None), "null output"),
             (lambda a: a.joint_map.__setitem__(3, 24), "joint_map[3] = 24 is no SMPL joint"),
             (lambda a: a.joint_map.__setitem__(3, a.joint_map[2]), "is taken twice"),
             (lambda a: a.parent_indices.__setitem__(0, 0), "body 0 must be the root"),
             (lambda a: a.parent_indices.__setitem__(4, 4), "parent_indices[4] = 4"), (lambda a: setattr(a, "num_envs", INVALID), "negative num_envs")]
    for change, message in cases:
        a = _args()
        change(a)
        assert lib.pulse_keypoint_push(ctypes.byref(a), None) != 0, message
        assert message in lib.pulse_last_error().decode(), (message, lib.pulse_last_error().decode())
