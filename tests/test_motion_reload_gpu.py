"""GPU: MotionLib.load_motions on a library built from raw motion data (MotionLibBase.load_motions, motion_lib_base.py:179-318) and
HumanoidIm.resample_motions on top of it: which clips become resident, the PMCP weights steering the draw, the launch signature, and
the env stepping in lockstep with the CPU twin fed the reloaded tables (pattern and tolerances of
tests/test_smplx_gpu.py:test_smplx_env_lockstep_with_cpu_twin: 1e-5 on observations and rewards, flags exact)."""
import numpy as np
import pytest
import torch

from oracle import env_oracle as E
from oracle.motion_oracle import OracleMotionLib
from pulse_amd import configs
from pulse_amd import synthetic as syn
from pulse_amd.env.motion_lib import MotionLib

pytestmark = pytest.mark.gpu
ATOL = 1e-5
FRAMES = [12, 20, 7, 33, 9, 15, 26, 4]
FPS = [30, 30, 60, 30, 30, 60, 30, 30]


@pytest.fixture()
def lib8(dev):
    """8 unique synthetic clips, 4 resident slots, 24 bodies."""
    g = syn.make_generator(4242)
    data, trees = syn.synthetic_motion_data(g, 8, frames=FRAMES, fps=FPS, num_slots=4)
    return MotionLib.from_motion_data(data, trees, device=dev, generator=g), data


def test_sequential_reload_wraps_around_the_data_set(lib8):
    lib, data = lib8
    keys = list(data)
    assert lib._num_unique_motions == 8 and lib.num_motions() == 4 and lib._motion_data_keys == keys
    lib.load_motions(random_sample=False, start_idx=6)
    want = [6, 7, 0, 1]
    assert lib._curr_motion_ids.cpu().tolist() == want and lib.curr_motion_keys == [keys[i] for i in want]
    nf = torch.tensor([FRAMES[i] for i in want])
    fps = torch.tensor([FPS[i] for i in want], dtype=torch.float64)
    assert torch.equal(lib._motion_num_frames.cpu(), nf) and torch.equal(lib._motion_fps.cpu(), fps.float())
    assert torch.equal(lib._motion_lengths.cpu(), ((nf - 1).double() / fps).float())                       # (F - 1) / fps
    assert torch.equal(lib.length_starts.cpu(), torch.tensor([0, 26, 30, 42])) and lib.frames.shape[0] == 62
    assert torch.equal(lib._sampling_batch_prob.cpu(), torch.full((4,), 0.25))
    assert torch.equal(lib.motion_ids.cpu(), torch.arange(4))


def test_hard_sampling_weight_steers_the_reloads(lib8):
    lib, data = lib8
    keys = list(data)
    lib.update_hard_sampling_weight([keys[2], keys[5]])
    seen = set()
    for _ in range(10):
        lib.load_motions()
        ids = lib._curr_motion_ids.cpu().tolist()
        assert set(ids) <= {2, 5}, ids
        assert set(lib.curr_motion_keys) <= {keys[2], keys[5]}
        assert torch.allclose(lib._sampling_batch_prob.sum().cpu(), torch.tensor(1.0))
        seen.update(ids)
    assert seen == {2, 5}, "40 draws from two equally likely clips never produced one of them"


def test_reload_changes_the_launch_signature(lib8):
    lib, _ = lib8
    sig, ptr = lib.launch_signature(), lib.frames.data_ptr()
    old = lib.frames
    lib.load_motions()
    assert lib.launch_signature() != sig and lib.frames is not old and lib.frames.data_ptr() != ptr


def test_max_len_crops_inside_the_clip(lib8):
    lib, data = lib8
    keys = list(data)
    lib.load_motions(random_sample=False, start_idx=0, max_len=10)                                      # clips of 12, 20, 7, 33 frames
    assert lib._motion_num_frames.cpu().tolist() == [10, 10, 7, 10]
    assert torch.equal(lib._motion_lengths.cpu(), (torch.tensor([9, 9, 6, 9]).double() / torch.tensor([30, 30, 60, 30]).double()).float())
    # im_eval: longest first and no heading, so grs is the staged input: every cropped window must be found in its source clip
    ev = MotionLib.from_motion_data(data, lib._last_load["skeleton_trees"], device=lib._device, im_eval=True, generator=syn.make_generator(5))
    assert ev._motion_data_keys == sorted(keys, key=lambda k: -data[k]["pose_quat_global"].shape[0]) and ev.motion_heading is None
    ev.load_motions(random_sample=False, start_idx=0, max_len=10)                                       # 33, 26, 20, 15 frames
    starts = ev.length_starts.cpu().tolist()
    for slot, k in enumerate(ev.curr_motion_keys):
        src = torch.as_tensor(data[k]["pose_quat_global"])
        got = ev.grs[starts[slot]:starts[slot] + 10].cpu()
        hits = [s for s in range(src.shape[0] - 9) if torch.equal(src[s:s + 10], got)]
        assert len(hits) == 1, f"slot {slot} ({k}): the cropped records are no window of the clip"


def _expected_step(task, lib, ids):
    """The row HumanoidIm must have produced from the state the device holds now (read back): reference at t and t + 1 from the CPU
    motion library, reward / reset by env_oracle.post_physics, the observation by the oracle's general forms."""
    c = lambda x: x.detach().cpu().clone()
    rb, prog = c(task.sim.rigid_body_state), c(task.progress_buf)
    start, start_off, off = c(task._motion_start_times), c(task._motion_start_times_offset), c(task._global_offset)
    t_now = prog * task.dt + start + start_off
    t_next = (prog + 1) * task.dt + start + start_off
    ref = lambda s: {"pos": s["rg_pos"], "rot": s["rb_rot"], "vel": s["body_vel"], "ang": s["body_ang_vel"]}
    now, nxt = ref(lib.get_motion_state(ids, t_now, off)), ref(lib.get_motion_state(ids, t_next, off))
    pass_time = t_now >= lib.get_motion_length(ids)
    rid, tid = c(task._reset_bodies_id).long().tolist(), c(task._track_bodies_id).long().tolist()
    pp = E.post_physics(rb, now, nxt, c(task.sim.dof_force), c(task.sim.dof_vel), prog, pass_time, rid, tid, c(task._termination_distances)[None],
                        cycle_counter=c(task._cycle_counter))
    bp, br, bv, ba = E.split_rb(rb)
    up = task._has_upright_start
    obs = torch.cat([E.self_obs_smpl_max_general(bp, br, bv, ba, upright=up),
                     E.im_obs_variant(6, bp[:, 0], br[:, 0], bp[:, tid], br[:, tid], bv[:, tid], ba[:, tid], nxt["pos"][:, tid], nxt["rot"][:, tid],
                                      nxt["vel"][:, tid], nxt["ang"][:, tid], 1, up)], dim=-1)
    return obs, pp


def close(got, want, name, atol=ATOL):
    got, want = got.detach().cpu().numpy().astype(np.float64), want.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, f"{name}: {got.shape} vs {want.shape}"
    err = np.abs(got - want)
    print(f"{name}: max abs error {err.max():.3e}")
    assert np.isfinite(got).all() and err.max() <= atol, f"{name}: max abs error {err.max():.3e} > {atol}"


def _lockstep(env, task, steps, nd, g, tag):
    lib = OracleMotionLib(task._motion_lib.tables())
    ids = task._sampled_motion_ids.cpu()
    for k in range(steps):
        obs, rew, done, info = env.step(torch.randn(task.num_envs, nd, generator=g).to(task.device))
        want, pp = _expected_step(task, lib, ids)
        close(obs, want, f"{tag} obs step {k}")
        close(rew, pp["rew"], f"{tag} rew step {k}")
        close(info["reward_raw"], pp["raw"], f"{tag} reward_raw step {k}")
        assert torch.equal(done.cpu(), pp["reset"]), f"{tag} reset flags step {k}"
        assert torch.equal(info["terminate"].cpu(), pp["terminate"]), f"{tag} terminate step {k}"
        hit = torch.nonzero(pp["reset"]).flatten()
        if hit.numel():
            obs = env.reset(hit.to(task.device))
            want, _ = _expected_step(task, lib, ids)
            close(obs.cpu()[hit], want[hit], f"{tag} obs after reset {k}")


@pytest.mark.parametrize("humanoid", ["smpl", "smplx"])
def test_env_resamples_motions_and_stays_in_lockstep(dev, humanoid):
    n = 16
    env, _ = configs.make_env(n, 12, dev, seed=99, reference="motion_data", humanoid=humanoid)
    task = env.task
    mlib = task._motion_lib
    assert mlib.reloads and mlib.num_motions() == n and mlib._num_unique_motions == 9 and mlib.num_bodies == task.num_bodies
    nd = task.num_actions
    g = torch.Generator().manual_seed(1)
    obs = env.reset()
    want, _ = _expected_step(task, OracleMotionLib(mlib.tables()), task._sampled_motion_ids.cpu())
    close(obs, want, "obs after the first reset")
    _lockstep(env, task, 4, nd, g, "before")
    sig, keys_before, frames_before = mlib.launch_signature(), list(mlib.curr_motion_keys), mlib.frames
    task.resample_motions()
    assert mlib.launch_signature() != sig and mlib.frames is not frames_before
    assert (task.progress_buf == 0).all(), "resample_motions restarts every env"
    assert torch.equal(task._motion_len_env.cpu(), mlib.get_motion_length(task._sampled_motion_ids).cpu())
    want, _ = _expected_step(task, OracleMotionLib(mlib.tables()), task._sampled_motion_ids.cpu())
    close(task.obs_buf, want, "obs after resample_motions")
    _lockstep(env, task, 4, nd, g, "after")
    assert len(keys_before) == n and len(mlib.curr_motion_keys) == n
