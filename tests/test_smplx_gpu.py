"""GPU: the 52-body SMPL-X / SMPL-H humanoid on the imitation step, the motion query, the env and the agent.

pulse_im_step and pulse_motion_state map lane = body; past 32 bodies they take a whole wave per (env, role) / per query.  Every
step launch here runs with PULSE_IM_DEBUG_POISON_LDS (LDS pre-filled with NaN: a read of a word nobody wrote shows in the output).

Tolerances: 1e-5 absolute on observations and rewards, the project's figure for these outputs at 24 bodies -- the inputs have the same
distribution and every output is a per-body expression or a mean over bodies, so the bound carries over; reset / terminate exact
(the inputs keep every distance at least 1e-4 from the threshold, asserted).  The yardsticks are tests/golden/env_smplx.npz (the
reference's own functions, tools/gen_golden_smplx.py) and oracle/env_oracle.py, which tests/test_smplx_cpu.py ties to that fixture
bit for bit."""
import os

import numpy as np
import pytest
import torch

from oracle import env_oracle as E
from oracle.motion_oracle import OracleMotionLib
from pulse_amd import _lib, configs, ops
from pulse_amd import synthetic as syn
from pulse_amd._lib import PULSE_IM_DEBUG_POISON_LDS as POISON
from pulse_amd._lib import PULSE_IM_FORCE_WIDE, PULSE_IM_RESET, PULSE_IM_REWARD, PULSE_IM_SELF_OBS, PULSE_IM_TASK_OBS
from test_smplx_cpu import load_generator

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = PULSE_IM_SELF_OBS | PULSE_IM_TASK_OBS | PULSE_IM_REWARD | PULSE_IM_RESET
ATOL = 1e-5


@pytest.fixture(autouse=True)
def poison_lds(monkeypatch):
    monkeypatch.setattr(ops, "_IM_DEBUG_BITS", POISON)        # the env's own launches (ops.im_step ORs it into ``what``)


@pytest.fixture(scope="module")
def gen():
    return load_generator()


@pytest.fixture(scope="module")
def fx(gen):
    z = np.load(os.path.join(ROOT, "tests", "golden", "env_smplx.npz"))
    d = gen.inputs()
    for k, v in gen.input_sums(d).items():
        assert v.item() == z[k].item(), k
    return z, d


def close(got, want, name, atol=ATOL):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else want
    assert got.shape == want.shape, f"{name}: {got.shape} vs {want.shape}"
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"{name}: max abs error {np.nanmax(err) if err.size else 0.0:.3e}")
    assert np.isfinite(got).all(), f"{name}: non-finite values (a read of poisoned LDS?)"
    assert err.max() <= atol, f"{name}: max abs error {err.max():.3e} > {atol}"


def step(dev, d, *, what=FULL, obs_v=6, T=1, upright=True, track=None, reset_ids, use_mean=False, term=0.25, rows=None, ref_next=None, **kw):
    """One arrays-mode launch of pulse_im_step on the inputs ``d`` (rows ``rows`` of them)."""
    sl = (lambda x: x) if rows is None else (lambda x: x[rows].contiguous())
    to = lambda x: sl(x).to(dev)
    rb = to(d["rb"])
    n, j = rb.shape[0], rb.shape[1]
    rx = d["ref_next"] if ref_next is None else ref_next
    slT = (lambda x: x) if rows is None else (lambda x: x.view(-1, T, *x.shape[1:])[rows].reshape(-1, *x.shape[1:]).contiguous())
    return ops.im_step(rb, what=what | POISON, ref_now={k: to(v) for k, v in d["ref_now"].items()}, ref_next={k: slT(v).to(dev) for k, v in rx.items()},
                       time_steps=T, dof_force=to(d["dof_force"]), dof_vel=to(d["dof_vel"]), progress=to(d["progress"]), pass_time=to(d["pass_time"]),
                       track_ids=list(range(j)) if track is None else track, reset_ids=reset_ids, term_dist=torch.full((j,), term, device=dev),
                       reset_use_mean=use_mean, obs_version=obs_v, upright=upright, **kw)


# ------------------------------------------------------------------------------------------------ 1. the step kernel vs the reference's outputs
VARIANTS = [(6, 1, True), (6, 1, False), (6, 3, True), (6, 3, False), (7, 1, True), (7, 1, False), (7, 3, True), (7, 3, False)]


def _fixture_case(z, d, gen, obs_v, T, upright):
    tag = "" if upright else "_noup"
    rx = d["ref_next"] if T == 3 else gen.first_sample(d["ref_next"], d["rb"].shape[0])
    if obs_v == 6 and f"v6_T{T}{tag}" not in z.files:
        # v6, three samples, upright: the one variant the fixture does not hold (file size).  The yardstick is the oracle, which
        # tests/test_smplx_cpu.py holds to the reference's function for this very case, bit for bit
        assert (T, upright) == (3, True)
        bp, br, bv, ba = E.split_rb(d["rb"])
        task = E.im_obs_variant(6, bp[:, 0], br[:, 0], bp, br, bv, ba, rx["pos"], rx["rot"], rx["vel"], rx["ang"], 3, True).numpy()
    else:
        task = z[f"v6_T{T}{tag}"] if obs_v == 6 else z[f"v7_T{T}_vr{tag}"]
    return np.concatenate([z["self_obs" + tag], task], axis=1), rx, (None if obs_v == 6 else gen.TRACK_VR)


@pytest.mark.parametrize("use_mean", [False, True])
@pytest.mark.parametrize("obs_v,T,upright", VARIANTS)
def test_step_kernel_matches_reference_outputs(dev, fx, gen, obs_v, T, upright, use_mean):
    z, d = fx
    want_obs, rx, track = _fixture_case(z, d, gen, obs_v, T, upright)
    out = step(dev, d, obs_v=obs_v, T=T, upright=upright, track=track, reset_ids=gen.RESET_IDS, use_mean=use_mean, ref_next=rx)
    assert out["obs"].shape == want_obs.shape
    close(out["obs"], want_obs, "obs")
    close(out["rew"], z["reward"], "rew")
    close(out["rew_raw"], z["reward_raw"], "rew_raw")
    mt = "_mean" if use_mean else ""
    assert np.array_equal(out["reset"].cpu().numpy(), z["reset" + mt]) and np.array_equal(out["terminate"].cpu().numpy(), z["terminate" + mt])


def test_step_kernel_row_pitch_and_pad(dev, fx, gen):
    """The SMPL-X row of the env: 2026 columns written into a 2048-float pitch, pad zeroed, nothing past it touched."""
    z, d = fx
    want_obs, rx, _ = _fixture_case(z, d, gen, 6, 1, False)
    n = want_obs.shape[0]
    store = torch.full((n, 2080), 7.0, device=dev)
    step(dev, d, upright=False, reset_ids=gen.RESET_IDS, ref_next=rx, obs=store, obs_cols=2048)
    close(store[:, :2026], want_obs, "obs")
    assert (store[:, 2026:2048] == 0).all() and (store[:, 2048:] == 7.0).all()


@pytest.mark.parametrize("obs_v,T,upright", [(6, 3, False), (7, 1, True)])
def test_step_kernel_partial_workgroups(dev, fx, gen, obs_v, T, upright):
    """env_ids selecting 5 of the 33 envs (the others' outputs stay untouched) and a single env: workgroups that are not full."""
    z, d = fx
    want_obs, rx, track = _fixture_case(z, d, gen, obs_v, T, upright)
    n, w = want_obs.shape
    ids = torch.tensor([32, 3, 17, 0, 21], device=dev)
    bufs = dict(obs=torch.full((n, w), -3.0, device=dev), rew=torch.full((n,), -3.0, device=dev), rew_raw=torch.full((n, 5), -3.0, device=dev),
                reset=torch.full((n,), -3, dtype=torch.int64, device=dev), terminate=torch.full((n,), -3, dtype=torch.int64, device=dev))
    step(dev, d, obs_v=obs_v, T=T, upright=upright, track=track, reset_ids=gen.RESET_IDS, ref_next=rx, env_ids=ids, **bufs)
    sel = ids.cpu().numpy()
    rest = np.setdiff1d(np.arange(n), sel)
    close(bufs["obs"][ids], want_obs[sel], "obs[env_ids]")
    close(bufs["rew"][ids], z["reward"][sel], "rew[env_ids]")
    close(bufs["rew_raw"][ids], z["reward_raw"][sel], "rew_raw[env_ids]")
    assert np.array_equal(bufs["reset"].cpu().numpy()[sel], z["reset"][sel]) and np.array_equal(bufs["terminate"].cpu().numpy()[sel], z["terminate"][sel])
    for k, v in bufs.items():
        assert (v.cpu()[rest] == -3).all(), f"{k}: an env outside env_ids was written"
    out = step(dev, d, obs_v=obs_v, T=T, upright=upright, track=track, reset_ids=gen.RESET_IDS, ref_next=rx, rows=slice(0, 1))
    close(out["obs"], want_obs[:1], "obs[n=1]")
    close(out["rew"], z["reward"][:1], "rew[n=1]")
    assert np.array_equal(out["reset"].cpu().numpy(), z["reset"][:1]) and np.array_equal(out["terminate"].cpu().numpy(), z["terminate"][:1])


# ------------------------------------------------------------------------------------------------ 2. body-count edges vs the oracle
@pytest.mark.parametrize("j", [33, 52, 64])       # the first count past the half-wave, SMPL-X, the full wave
def test_body_count_edges_match_oracle(dev, gen, j):
    n = 7
    d = gen.inputs(n=n, j=j, seed=9000 + j, samples=1)
    reset_ids = [b for b in range(j) if b % 3 != 2]                       # two bodies in three: 22 / 35 / 43 of them, past 32 at 52 and 64 bodies
    term = torch.full((1, j), gen.TERM_DIST)
    want = E.post_physics(d["rb"], d["ref_now"], d["ref_next"], d["dof_force"], d["dof_vel"], d["progress"], d["pass_time"], reset_ids, list(range(j)), term)
    dist = torch.norm(d["rb"][:, reset_ids, 0:3] - d["ref_now"]["pos"][:, reset_ids], dim=-1)
    gen.check_conditions(want["raw"], want["terminate"], torch.cat([dist.flatten(), dist.mean(dim=-1)]))
    for use_mean in (False, True):
        w = want if not use_mean else E.post_physics(d["rb"], d["ref_now"], d["ref_next"], d["dof_force"], d["dof_vel"], d["progress"], d["pass_time"],
                                                     reset_ids, list(range(j)), term, use_mean=True)
        out = step(dev, d, reset_ids=reset_ids, use_mean=use_mean)
        assert out["obs"].shape == (n, 15 * j - 2 + 24 * j)
        close(out["obs"], w["obs"], "obs")
        close(out["rew"], w["rew"], "rew")
        close(out["rew_raw"], w["raw"], "rew_raw")
        assert torch.equal(out["reset"].cpu(), w["reset"]) and torch.equal(out["terminate"].cpu(), w["terminate"])


@pytest.mark.parametrize("upright", [True, False])
def test_self_observation_versions_at_52_bodies(dev, upright):
    n, j, h = 9, 52, 4
    g = syn.make_generator(77)
    hist = syn.rigid_body_state(g, n * h, j).view(n, h, j, 13)
    fs = torch.randn(n, 12, generator=g)
    sp = lambda x: (x[..., 0:3].contiguous(), x[..., 3:7].contiguous(), x[..., 7:10].contiguous(), x[..., 10:13].contiguous())
    got = ops.im_step(hist.to(dev), what=PULSE_IM_SELF_OBS | POISON, self_obs_version=2, upright=upright)["obs"]
    close(got, E.self_obs_smpl_max_v2(*sp(hist), upright=upright), "self_obs_v2")
    rb = hist[:, -1].contiguous()
    got = ops.im_step(rb.to(dev), what=PULSE_IM_SELF_OBS | POISON, self_obs_version=3, force_sensor=fs.to(dev), upright=upright)["obs"]
    close(got, E.self_obs_smpl_max_general(*sp(rb), upright=upright, force_sensor=fs), "self_obs_v3")
    assert got.shape == (n, 778 + 12)


# ------------------------------------------------------------------------------------------------ 3. the wide form is the same arithmetic
@pytest.mark.parametrize("what", [FULL, PULSE_IM_REWARD | PULSE_IM_RESET, PULSE_IM_SELF_OBS | PULSE_IM_TASK_OBS])
@pytest.mark.parametrize("obs_v,track", [(6, None), (7, syn.VR_TRACK_BODY_IDS)])
def test_wide_form_is_bit_identical_at_24_bodies(dev, golden, what, obs_v, track):
    """At <= 32 bodies the upper 32 lanes of a 64-lane group feed exact zeros into every butterfly: a difference between the two forms is a
    lane-index or staging error, not rounding."""
    z = golden("env_im.npz")
    d = {"rb": z.t("rb"), "dof_force": z.t("dof_force"), "dof_vel": z.t("dof_vel"), "progress": z.t("progress"), "pass_time": z.t("pass_time"),
         "ref_now": {k: z.t("ref_now_" + k) for k in ("pos", "rot", "vel", "ang")}, "ref_next": {k: z.t("ref_next_" + k) for k in ("pos", "rot", "vel", "ang")}}
    for use_mean in (False, True):
        a = step(dev, d, what=what, obs_v=obs_v, track=track, reset_ids=syn.RESET_BODY_IDS, use_mean=use_mean)
        b = step(dev, d, what=what | PULSE_IM_FORCE_WIDE, obs_v=obs_v, track=track, reset_ids=syn.RESET_BODY_IDS, use_mean=use_mean)
        assert sorted(a) == sorted(b) and len(a) >= 1
        for k in a:
            assert torch.isfinite(a[k].float()).all(), k
            assert torch.equal(a[k], b[k]), f"{k}: the 64-lane form differs from the 32-lane form"
    if what == FULL and obs_v == 6:                   # and both are the kernel the 24-body golden pins
        close(a["obs"], np.concatenate([z.np("self_obs"), z.np("task_obs_v6")], axis=1), "obs vs env_im.npz")


def test_more_than_32_reset_ids_at_24_bodies_take_the_wide_form(dev, golden):
    """The launcher's width rule (include/pulse_hip.h): lane = reset id in the reset stage, so more than 32 reset ids (repeats, at <= 32
    bodies) take the 64-lane form too.  Every id twice: the any-body-fell flags and every other output equal the 20-id launch."""
    z = golden("env_im.npz")
    d = {"rb": z.t("rb"), "dof_force": z.t("dof_force"), "dof_vel": z.t("dof_vel"), "progress": z.t("progress"), "pass_time": z.t("pass_time"),
         "ref_now": {k: z.t("ref_now_" + k) for k in ("pos", "rot", "vel", "ang")}, "ref_next": {k: z.t("ref_next_" + k) for k in ("pos", "rot", "vel", "ang")}}
    a = step(dev, d, reset_ids=syn.RESET_BODY_IDS)
    b = step(dev, d, reset_ids=syn.RESET_BODY_IDS + syn.RESET_BODY_IDS[::-1])
    assert len(syn.RESET_BODY_IDS) * 2 == 40
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert np.array_equal(b["reset"].cpu().numpy(), z.np("reset")) and np.array_equal(b["terminate"].cpu().numpy(), z.np("terminate")) and z.np("terminate").any()
    with pytest.raises(_lib.PulseLibraryError, match="reset ids"):
        step(dev, d, reset_ids=list(range(24)) * 3)                      # 72 > 64


# ------------------------------------------------------------------------------------------------ 4. motion query
def _binary_tree(j):
    return {"parents": [-1] + [(b - 1) // 2 for b in range(1, j)]}


@pytest.mark.parametrize("humanoid", ["smplx", 33, 64])
def test_motion_query_matches_oracle(dev, humanoid):
    from pulse_amd.env.motion_lib import MotionLib
    sk = syn.skeleton(humanoid) if isinstance(humanoid, str) else _binary_tree(humanoid)
    j = len(sk["parents"])
    g = syn.make_generator(2)
    tabs = syn.synthetic_motion_library(g, 5, 12, 30, humanoid=sk)
    ids = torch.randint(0, 5, (97,), generator=g)
    times = torch.rand(97, generator=g) * tabs["motion_lengths"][ids]
    off = torch.randn(97, 3, generator=g)
    lib = MotionLib.from_tables(tabs, dev)
    assert lib.frame_stride % 4 == 0 and lib.offsets["grs"] % 4 == 0 and lib.offsets["lrs"] % 4 == 0
    if j == 52:
        assert lib.frame_stride == 1040 and lib.num_dof == 153
    got = lib.get_motion_state(ids.to(dev), times.to(dev), off.to(dev))
    want = OracleMotionLib(tabs).get_motion_state(ids, times, off)
    assert got["rg_pos"].shape == (97, j, 3) and got["dof_pos"].shape == (97, 3 * (j - 1))
    for k in ("rg_pos", "body_vel", "body_ang_vel", "dof_vel", "root_pos", "root_vel", "root_ang_vel"):        # lerps: bit for bit, as at 24 bodies
        assert torch.equal(got[k].cpu(), want[k]), k
    for k in ("rb_rot", "root_rot", "dof_pos"):                                                                 # slerp / exp map: 2e-6, as at 24 bodies
        close(got[k], want[k], k, atol=2e-6)
    rec = lib.query(ids.to(dev), times.to(dev), off.to(dev), fields=("rb_records",))["rb_records"]
    assert torch.equal(rec, torch.cat([got["rg_pos"], got["rb_rot"], got["body_vel"], got["body_ang_vel"]], dim=-1))


# ------------------------------------------------------------------------------------------------ 5. the env in library mode, lockstep
def _expected_step(task, lib, ids):
    """The row HumanoidIm must have produced from the state the device holds now (read back): reference at t and t + 1 from the CPU
    motion library, reward / reset by env_oracle.post_physics, the non-upright observation by the oracle's general forms."""
    c = lambda x: x.detach().cpu().clone()
    rb, prog = c(task.sim.rigid_body_state), c(task.progress_buf)
    start, start_off, off = c(task._motion_start_times), c(task._motion_start_times_offset), c(task._global_offset)
    t_now = prog * task.dt + start + start_off
    t_next = (prog + 1) * task.dt + start + start_off
    ref = lambda s: {"pos": s["rg_pos"], "rot": s["rb_rot"], "vel": s["body_vel"], "ang": s["body_ang_vel"]}
    now, nxt = ref(lib.get_motion_state(ids, t_now, off)), ref(lib.get_motion_state(ids, t_next, off))
    j = rb.shape[1]
    pass_time = t_now >= lib.get_motion_length(ids)
    rid, tid = c(task._reset_bodies_id).long().tolist(), c(task._track_bodies_id).long().tolist()
    pp = E.post_physics(rb, now, nxt, c(task.sim.dof_force), c(task.sim.dof_vel), prog, pass_time, rid, tid, c(task._termination_distances)[None],
                        cycle_counter=c(task._cycle_counter))
    bp, br, bv, ba = E.split_rb(rb)
    obs = torch.cat([E.self_obs_smpl_max_general(bp, br, bv, ba, upright=False),
                     E.im_obs_variant(6, bp[:, 0], br[:, 0], bp[:, tid], br[:, tid], bv[:, tid], ba[:, tid], nxt["pos"][:, tid], nxt["rot"][:, tid],
                                      nxt["vel"][:, tid], nxt["ang"][:, tid], 1, False)], dim=-1)
    assert j == 52
    return obs, pp


def test_smplx_env_lockstep_with_cpu_twin(dev):
    n, horizon, seed = 64, 20, 321
    env, _ = configs.make_env(n, horizon, dev, seed=seed, reference="motion_lib", humanoid="smplx")
    task = env.task
    assert task.humanoid_type == "smplx" and task.num_bodies == 52 and not task._has_upright_start
    assert task.num_obs == 2026 and task.obs_pitch == 2048 and task.num_actions == 153
    assert task._reset_bodies_id.numel() == 48 and task._track_bodies_id.numel() == 52
    lib = OracleMotionLib(syn.synthetic_motion_library(syn.make_generator(seed + 5, 0), n, humanoid="smplx"))
    ids = task._sampled_motion_ids.cpu()
    obs = env.reset()
    want, _ = _expected_step(task, lib, ids)
    close(obs, want, "obs after the first reset")
    g = torch.Generator().manual_seed(1)
    n_done = 0
    for k in range(horizon):
        obs, rew, done, info = env.step(torch.randn(n, 153, generator=g).to(dev))
        want, pp = _expected_step(task, lib, ids)
        close(obs, want, f"obs step {k}")
        close(rew, pp["rew"], f"rew step {k}")
        close(info["reward_raw"], pp["raw"], f"reward_raw step {k}")
        assert torch.equal(done.cpu(), pp["reset"]), f"reset flags step {k}"
        assert torch.equal(info["terminate"].cpu(), pp["terminate"]), f"terminate step {k}"
        hit = torch.nonzero(pp["reset"]).flatten()
        n_done += hit.numel()
        if hit.numel():
            obs = env.reset(hit.to(dev))
            assert (task.progress_buf.cpu()[hit] == 0).all()
            want, _ = _expected_step(task, lib, ids)
            close(obs.cpu()[hit], want[hit], f"obs after reset {k}")
    assert n_done > 0, "the lockstep run never exercised a reset"


def test_smplx_env_on_recorded_frames(dev):
    """The other reference source: pre-recorded 52-body frames (RecordedRollout / RecordedSim / RecordedMotion take the skeleton)."""
    n = 9
    env, ro = configs.make_env(n, 4, dev, seed=3, humanoid="smplx")
    task = env.task
    assert ro.data["rb"].shape[1:] == (n, 52, 13) and task.sim.dof_vel.shape == (n, 153) and task.num_obs == 2026
    env.reset()
    obs, rew, done, info = env.step(torch.zeros(n, 153, device=dev))
    f = task.sim.frame
    c = lambda x: x.detach().cpu()
    rb, rn, rx = c(ro.data["rb"][f]), {k: c(v[f]) for k, v in ro.ref_now.items()}, {k: c(v[f]) for k, v in ro.ref_next.items()}
    rid, tid = c(task._reset_bodies_id).long().tolist(), list(range(52))
    pp = E.post_physics(rb, rn, rx, c(ro.data["dof_force"][f]), c(ro.data["dof_vel"][f]), c(task.progress_buf), c(task._pass_time), rid, tid,
                        c(task._termination_distances)[None])
    bp, br, bv, ba = E.split_rb(rb)
    want = torch.cat([E.self_obs_smpl_max_general(bp, br, bv, ba, upright=False),
                      E.im_obs_variant(6, bp[:, 0], br[:, 0], bp, br, bv, ba, rx["pos"], rx["rot"], rx["vel"], rx["ang"], 1, False)], dim=-1)
    close(obs, want, "obs")
    close(rew, pp["rew"], "rew")
    assert torch.equal(done.cpu(), pp["reset"]) and torch.equal(info["terminate"].cpu(), pp["terminate"])


# ------------------------------------------------------------------------------------------------ 6. the agent
def test_smplx_agent_trains_and_restores(dev):
    torch.manual_seed(3)
    ag, _ = configs.make_agent("smplx_small", device=dev, seed=5, reference="motion_lib")
    task = ag.vec_env.env.task
    assert task.humanoid_type == "smplx" and task.get_obs_size() == 2026 and ag.actions_num == 153 and ag.model.in_pitch == 2048
    before = ag.model.flat.clone()
    info = ag.train_epoch()
    for k, v in info.items():
        if isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
            assert torch.isfinite(torch.stack([x.float().mean() for x in v])).all(), f"{k} is not finite"
    assert torch.isfinite(torch.stack(info["actor_loss"])).all() and torch.isfinite(torch.stack(info["critic_loss"])).all()
    assert info["grad_norm"][0].item() > 0
    assert not torch.equal(before, ag.model.flat), "one epoch left the parameters where they were"
    assert torch.isfinite(ag.model.flat).all()
    weights = ag.get_full_state_weights()
    other, _ = configs.make_agent("smplx_small", device=dev, seed=11, reference="motion_lib")
    other.init_tensors()
    obs = {"obs": ag.obs["obs"] if isinstance(ag.obs, dict) else ag.obs}
    ag.set_eval()
    other.set_eval()
    mu_a = ag.get_action_values(obs)["mus"].clone()
    mu_other = other.get_action_values(obs)["mus"].clone()
    assert mu_a.shape == (64, 153) and not torch.equal(mu_a, mu_other)              # another seed: another policy ...
    other.set_full_state_weights(weights)
    mu_b = other.get_action_values(obs)["mus"].clone()
    assert torch.equal(mu_a, mu_b), "the restored agent does not reproduce the first one's actions"       # ... until the checkpoint is restored


# ------------------------------------------------------------------------------------------------ 7. rejections
def test_too_many_bodies_is_an_argument_error(dev):
    import ctypes
    lib = _lib.load()
    rb = torch.zeros(4, 65, 13, device=dev)
    rew, raw = torch.full((4,), 5.0, device=dev), torch.full((4, 5), 5.0, device=dev)
    a = _lib.ImStepArgs()
    a.rb, a.rb_env_stride, a.num_envs, a.num_bodies, a.what = rb.data_ptr(), 65 * 13, 4, 65, PULSE_IM_REWARD
    a.rew, a.rew_raw, a.time_steps = rew.data_ptr(), raw.data_ptr(), 1
    assert lib.pulse_im_step(ctypes.byref(a), None) == -1                  # PULSE_ERR_INVALID_ARG
    assert "num_bodies 65 not in [1,64]" in lib.pulse_last_error().decode()
    torch.cuda.synchronize()
    assert (rew == 5.0).all() and (raw == 5.0).all()                       # nothing was launched
    with pytest.raises(_lib.PulseLibraryError, match=r"\[1,64\]"):
        ops.im_step(rb, what=PULSE_IM_SELF_OBS)
    from pulse_amd.env.motion_lib import MotionLib
    tabs = syn.synthetic_motion_library(syn.make_generator(1), 2, 10, 12, humanoid={"parents": [-1] + list(range(64))})
    with pytest.raises(_lib.PulseLibraryError, match=r"num_bodies 65 not in \[1,64\]"):
        MotionLib.from_tables(tabs, dev).get_motion_state(torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(3, device=dev))
