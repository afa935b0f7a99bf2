"""GPU: pulse_keypoint_push against the fp64 restatement of the reference's statements (tests/keypoint_stream_model.py; tests/golden/keypoint_stream.npz,
tools/gen_golden_keypoint_stream.py), and the host side on top of it (KeypointStream, HumanoidImMCPDemo, CommonPlayer.track / track_motion).

Per step and field, over every element (the rule of tests/test_motion_ingest_gpu.py):

    |hip - expected| <= 4 * err_field

with ``expected`` the model's fp64 run and ``err_field`` the distance of its float32-staged run from it (max over the fixture, stored in it): the
error of an fp32 evaluation of the reference's own statements.  The figures are printed before they are asserted.  ``raw`` is a copy: bit for bit.
Every state and output buffer sits between poison-filled guard rows (0x7FC0DEAD) that must come back untouched; ``j3d`` is a strided view of a
NaN-filled buffer, which the binding declares it honours (unit inner stride).  Streams A (37 frames, history 30) and B (7 frames, history 4), 5 envs:
0.625 workgroups of eight envs, 25 of 32 lanes per env; after a per-env clear the two envs of a wave hold different L."""
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

import gen_golden_keypoint_stream as GK  # noqa: E402
import keypoint_stream_model as KM  # noqa: E402
from pulse_amd import configs, kernels, ops  # noqa: E402
from pulse_amd import synthetic as syn  # noqa: E402
from pulse_amd._lib import PULSE_IM_SELF_OBS, PULSE_IM_TASK_OBS  # noqa: E402
from pulse_amd.env.keypoint_stream import KeypointStream  # noqa: E402
from pulse_amd.env.motion_lib import MotionLib  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 2                                    # poison rows before and after every buffer
POISON = 0x7FC0DEAD                          # a NaN with a payload: any write shows
N, J = 5, 24


@pytest.fixture(scope="module")
def fx():
    return GK.load()


class Guarded:
    """The kernel's state and outputs, each the middle of a poison-filled allocation of N + 2 GUARD env rows."""

    def __init__(self, dev, history):
        self.h, self.dev = history, dev
        shapes = {"root_ring": (history, 3), "body_ring": (history, J, 3), "prev_pos": (J, 3), "pos": (J, 3), "vel": (J, 3), "raw": (J, 3), "count": ()}
        self.full, self.view = {}, {}
        for k, s in shapes.items():
            full = torch.full((N + 2 * GUARD,) + s, POISON, dtype=torch.int32, device=dev)
            self.full[k] = full
            self.view[k] = full[GUARD:GUARD + N] if k == "count" else full.view(torch.float32)[GUARD:GUARD + N]
        for k in ("root_ring", "body_ring", "prev_pos", "count"):          # a fresh stream: zero state; the outputs stay poison until written
            self.view[k].zero_()
        self.taps = torch.from_numpy(kernels.keypoint_taps(history=history)).float().to(dev)

    def push(self, frame, env_mask=None):
        big = torch.full((N + 2, J + 3, 5), float("nan"), device=self.dev)                     # j3d: a strided view of a NaN-filled buffer
        j3d = big[1:1 + N, 2:2 + J, 1:4]
        j3d.copy_(torch.from_numpy(frame))
        assert not j3d.is_contiguous() and j3d.stride(-1) == 1
        v = self.view
        kernels.keypoint_push(j3d, taps=self.taps, root_ring=v["root_ring"], body_ring=v["body_ring"], count=v["count"], prev_pos=v["prev_pos"],
                              pos=v["pos"], vel=v["vel"], raw=v["raw"], joint_map=syn.smpl_joint_map(), parents=syn.SMPL_PARENTS,
                              env_mask=None if env_mask is None else torch.as_tensor(env_mask, device=self.dev))
        return v["pos"].cpu().numpy(), v["vel"].cpu().numpy()

    def clear(self, mask):
        m = torch.as_tensor(mask, device=self.dev)
        self.view["count"].masked_fill_(m, 0)
        self.view["prev_pos"].masked_fill_(m[:, None, None], 0.0)

    def guards_untouched(self):
        torch.cuda.synchronize()
        for k, full in self.full.items():
            assert (full[:GUARD] == POISON).all() and (full[GUARD + N:] == POISON).all(), f"{k}: a guard row was written"

    def state(self):
        return {k: v.cpu().numpy().copy() for k, v in self.view.items()}


def held(got, want, err, name):
    got = np.asarray(got).astype(np.float64)
    worst = float(np.abs(got - want).max())
    print(f"{name}: max |hip - expected| {worst:.3e} = {worst / err:.2f} x err ({err:.3e})")
    assert np.isfinite(got).all(), name
    assert worst <= 4 * err, f"{name}: {worst:.3e} > 4 x {err:.3e}"
    return worst


@pytest.mark.parametrize("name", sorted(GK.STREAMS))
def test_kernel_against_the_fp64_model(dev, fx, name):
    frames, history = GK.STREAMS[name]
    g = Guarded(dev, history)
    jm = syn.smpl_joint_map()
    worst_p = worst_v = 0.0
    for t in range(frames):
        pos, vel = g.push(fx[f"j3d_{name}"][t])
        worst_p = max(worst_p, float(np.abs(pos - fx[f"pos64_{name}"][t]).max()))
        worst_v = max(worst_v, float(np.abs(vel - fx[f"vel64_{name}"][t]).max()))
        assert np.isfinite(pos).all() and np.isfinite(vel).all(), t
        assert np.array_equal(g.view["raw"].cpu().numpy().view(np.int32), fx[f"j3d_{name}"][t][:, jm].view(np.int32)), t      # raw: bit for bit
        if t == 0:                                                   # the first step: velocity pos / dt
            held(vel, fx[f"pos64_{name}"][0] / float(np.float32(1 / 30)), float(fx["err_vel"]), f"stream {name} first velocity vs pos / dt")
    err_p, err_v = float(fx["err_pos"]), float(fx["err_vel"])
    print(f"stream {name}: pos {worst_p:.3e} = {worst_p / err_p:.2f} x err_pos ({err_p:.3e}); vel {worst_v:.3e} = {worst_v / err_v:.2f} x err_vel ({err_v:.3e})")
    assert worst_p <= 4 * err_p and worst_v <= 4 * err_v
    g.guards_untouched()
    assert g.view["count"].tolist() == [frames] * N
    for k in ("pos", "vel", "raw", "root_ring", "body_ring", "prev_pos"):
        assert not (g.view[k].view(torch.int32) == POISON).any(), f"{k}: an element was not written"


def test_clear_gives_those_envs_their_own_history(dev, fx):
    j3d, history = fx["j3d_A"], 30
    g, plain = Guarded(dev, history), Guarded(dev, history)
    m = KM.StreamModel(N, history=history, dtype=np.float64)
    cleared = np.array([False, True, False, True, False])
    for t in range(20):
        if t == 13:                                                  # after frame 12
            g.clear(cleared)
            m.clear(cleared)
        pos, vel = g.push(j3d[t])
        ppos, pvel = plain.push(j3d[t])
        want_p, want_v = m.push(j3d[t])
        if t >= 13:
            held(pos[cleared], want_p[cleared], float(fx["err_pos"]), f"frame {t} cleared envs pos (L = {t - 12})")
            held(vel[cleared], want_v[cleared], float(fx["err_vel"]), f"frame {t} cleared envs vel")
        assert np.array_equal(pos[~cleared].view(np.int32), ppos[~cleared].view(np.int32)), t          # the rest: the uncleared run, bit for bit
        assert np.array_equal(vel[~cleared].view(np.int32), pvel[~cleared].view(np.int32)), t
    assert g.view["count"].tolist() == [20, 7, 20, 7, 20]
    g.guards_untouched()


def test_env_mask_leaves_an_env_untouched(dev, fx):
    j3d, history = fx["j3d_A"], 30
    g = Guarded(dev, history)
    m = KM.StreamModel(N, history=history, dtype=np.float64)
    mask = np.array([True, True, False, True, True])
    for t in range(12):
        skip = 5 <= t < 8
        before = g.state()
        pos, vel = g.push(j3d[t], env_mask=mask if skip else None)
        want_p, want_v = m.push(j3d[t], env_mask=mask if skip else None)
        if skip:
            after = g.state()
            for k in before:                                         # state and outputs of env 2: the same bits as before the push
                assert np.array_equal(before[k][2].view(np.int32), after[k][2].view(np.int32)), (t, k)
        held(pos, want_p, float(fx["err_pos"]), f"frame {t} pos (env 2 skipped: {skip})")
        held(vel, want_v, float(fx["err_vel"]), f"frame {t} vel")
    assert g.view["count"].tolist() == [12, 12, 9, 12, 12]
    g.guards_untouched()


def test_plain_demo_takes_positions_as_given(dev, fx):
    """HumanoidImDemo: stream.direct, close_distance 0.25, no far-direction clamp (env 4 sits 9 m from its reference)."""
    env, rollout = configs.make_env(N, 16, str(dev), env_kind="im_demo")
    task = env.task
    assert type(task).__name__ == "HumanoidImDemo" and task.close_distance == 0.25 and task.far_distance == float("inf") and task.zero_out_far
    env.reset()
    pos = torch.from_numpy(fx["pos_A"][5]).to(dev)
    vel = torch.from_numpy(fx["vel_A"][5]).to(dev)
    pos[0] = task.sim.rigid_body_state[0, :, 0:3] + 0.01                                         # env 0: within 0.25 m after the step's frame change too
    for t in range(2):
        ref = task.stream.direct(pos, vel)
        if t == 1:
            pos0 = rollout.data["rb"][(task.sim.frame + 1) % rollout.num_frames][0, :, 0:3] + 0.01   # the frame the step will load
            task.stream.direct(torch.cat([pos0[None], pos[1:]]), vel)
        env.step(torch.zeros(N, task.num_actions, device=dev))
        direct = ops.im_step(task.sim.rigid_body_state, what=PULSE_IM_SELF_OBS | PULSE_IM_TASK_OBS, ref_next=ref, obs_version=7,
                             track_ids=task._track_bodies_id, upright=True, obs_cols=task.obs_pitch,
                             zero_out_far={"point_goal": torch.zeros(N, device=dev), "close_distance": 0.25, "far_distance": float("inf")})
        assert torch.equal(task.obs_buf.view(torch.int32), direct["obs"][:, :task.num_obs].view(torch.int32)), t
        assert torch.isfinite(task.obs_buf).all()
        assert not task.rew_buf.any() and not task.reset_buf.any() and not task._terminate_buf.any()
    d = (task.sim.rigid_body_state[:, 0, 0:3] - task.stream.pos[:, 0]).norm(dim=-1)
    assert float(d[0]) < 0.25 and float(d.max()) > 3.0                                           # both sides of close_distance, and beyond any clamp


def test_mcp_demo_env_and_player(dev, fx):
    env, _ = configs.make_env(N, 16, str(dev), env_kind="mcp_demo")
    task = env.task
    assert type(task).__name__ == "HumanoidImMCPDemo" and task.close_distance == 0.5 and task.zero_out_far and not task.zero_out_far_train
    assert isinstance(task.stream, KeypointStream) and task.obs_v == 7
    env.reset()
    for t in range(3):
        task.push_keypoints(torch.from_numpy(fx["j3d_A"][t]).to(dev))
        env.step(torch.zeros(N, task.num_actions, device=dev))
        got = task.obs_buf.clone()
        ref = task.stream.next()
        assert ref["pos"].data_ptr() == task.stream.pos.data_ptr()                               # the same storage every step
        direct = ops.im_step(task.sim.rigid_body_state, what=PULSE_IM_SELF_OBS | PULSE_IM_TASK_OBS, ref_next=ref, obs_version=7,
                             track_ids=task._track_bodies_id, upright=True, obs_cols=task.obs_pitch,
                             zero_out_far={"point_goal": torch.zeros(N, device=dev), "close_distance": 0.5, "far_distance": task.far_distance})
        assert torch.equal(got.view(torch.int32), direct["obs"][:, :task.num_obs].view(torch.int32)), t
        assert not task.rew_buf.any() and not task.reset_buf.any() and not task._terminate_buf.any()
        assert task.progress_buf.tolist() == [t + 1] * N
    # the player: 12 tracked steps, one push launch per frame, no reset; the tracked motion is a motion library
    envs, steps = 8, 12
    player = configs.make_player("mcp_demo_small", device=str(dev), num_envs_override=envs, minibatch_size=16 * envs)
    frames = torch.from_numpy(np.concatenate([fx["j3d_A"][:steps], fx["j3d_A"][:steps, :3]], axis=1)).to(dev)      # (12, 8, 24, 3)
    counted = []
    inner = kernels._launch
    kernels._launch = lambda name, *a, **k: (counted.append(name), inner(name, *a, **k))[1]
    try:
        run = player.track(frames)
        assert counted.count("pulse_keypoint_push") == steps, counted
        counted.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = player.track_motion(list(frames))                                              # an iterable of frames
        assert counted.count("pulse_keypoint_push") == steps and counted.count("pulse_motion_export") == 1, counted
    finally:
        kernels._launch = inner
    assert run["steps"] == steps and run["resets"] == 0
    assert len(out) == envs and all(c["pose_quat_global"].shape == (steps, 24, 4) for c in out.values())
    lib = MotionLib.from_motion_data(out, (syn.SMPL_PARENTS, torch.zeros(len(out), 24, 3)), device=dev, im_eval=True)
    lib.load_motions(random_sample=False)
    assert sorted(lib.curr_motion_keys) == sorted(out)
    t = player.env.task
    assert not t.reset_buf.any() and not t._terminate_buf.any() and not t.rew_buf.any() and int(t.stream.count[0]) == 2 * steps
