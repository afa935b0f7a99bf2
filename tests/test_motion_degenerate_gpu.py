"""GPU: the kernels that read the packed motion records through csrc/motion_math.h -- pulse_motion_state (32- and 64-lane forms, clock,
reset, root_only, rb_records modes), pulse_amp_hist_init, the in-kernel reference of pulse_im_step, pulse_task_ref_state_init, and
pulse_motion_build as the writer of such records -- on clips where slerp takes its OTHER outcomes: the sign flip, the midpoint fallback,
q0 itself, and the masked branch of quat_to_angle_axis behind them.  Still, frozen, identity, slow and sign-flipped joints, clips of 2 and
3 frames, queried at t = 0, t = length and every exact frame time (oracle/degenerate_clips.py).

References: tests/golden/motion_degenerate.npz (the reference's own get_motion_state; tests/test_motion_degenerate_cpu.py proves every
pair and query of it stable under the reference alone) and OracleMotionLib / the plain-torch models the suite already holds these kernels
to.  Tolerances are the suite's existing ones: lerped fields, frame indices and blend bit for bit, slerp / exp-map fields 2e-6
(tests/test_motion_lib.py); AMP frames 1e-5 (tests/test_amp_variants_gpu.py); transformed reset states 1e-5 (tests/test_task_reset_gpu.py);
pulse_slerp 5e-6 and pulse_quat_mul 2e-6 (test_rotation_ops_vs_golden).  Libraries have 8 clips of at most 17 frames.  No query is left
out anywhere; the one exception at cell level is stated at test_built_records_query_like_the_oracle (25 (query, joint) cells of dof_pos
held up to the sign of the wrap at pi)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import amp_frame_model as AM
import task_reset_model as TM
from oracle import degenerate_clips as D
from oracle import rotations as R
from oracle.motion_oracle import OracleMotionLib
from pulse_amd import ops, synthetic as syn
from pulse_amd.env.motion_lib import MotionLib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "motion_degenerate.npz")
EXACT = ("rg_pos", "body_vel", "body_ang_vel", "dof_vel", "root_pos", "root_vel", "root_ang_vel")
ROT = ("rb_rot", "root_rot", "dof_pos")
FIELDS = ("rg_pos", "rb_rot", "body_vel", "body_ang_vel", "dof_pos", "dof_vel", "rb_records")
SEED = 11
_shared = {}


def fixture():
    if "fx" not in _shared:
        _shared["fx"] = D.load_fixture(GOLDEN)
    return _shared["fx"]


def library(humanoid):
    """(tables, info, ids, times, offset, want) of a tree: the committed fixture for 'smpl', a build of the same clips elsewhere; the
    queries with one more appended so that n = 4 k + 1 (a partial last workgroup in both forms), the oracle's answer computed once."""
    if humanoid not in _shared:
        if humanoid == "smpl":
            z, tabs, info = fixture()
            ids, times, off = (torch.from_numpy(z[k]) for k in ("motion_ids", "motion_times", "offset"))
        else:
            tabs, info = D.build(SEED, humanoid)
            ids, times, off = D.queries(tabs, SEED)
        ids, times, off = torch.cat([ids, ids[:1]]), torch.cat([times, times[:1]]), torch.cat([off, off[:1]])
        assert ids.numel() % 4 == 1 and ids.numel() % 8 != 0
        assert D.unstable_pairs(tabs) == [] and D.query_conditions(tabs, ids, times) == []
        _shared[humanoid] = (tabs, info, ids, times, off, OracleMotionLib(tabs).get_motion_state(ids, times, off))
    return _shared[humanoid]


def compare(res, want, keys_exact=EXACT, keys_rot=ROT):
    for k in keys_exact:
        assert torch.equal(res[k].cpu(), want[k]), k
    for k in keys_rot:
        np.testing.assert_allclose(res[k].cpu().numpy(), want[k].numpy(), atol=2e-6, rtol=0, err_msg=k)


def kind_properties(tabs, info, ids, got, what):
    """What holds exactly whatever the rounding: dof_pos of an identity joint is zero, dof_pos of a frozen joint has the same bits on every
    query of its clip, rb_rot of the wholly still clip is the stored rotation."""
    kinds = torch.from_numpy(info["kinds"])
    n = ids.numel()
    dof = got["dof_pos"].cpu().view(n, -1, 3)
    ident = (kinds[ids][:, 1:] == D.IDENTITY)
    assert ident.any() and (dof[ident] == 0).all(), f"{what}: dof_pos of an identity joint is not exactly zero"
    seen = 0
    for m in range(kinds.shape[0]):
        rows = dof[ids == m].view(torch.int32)
        frozen = (kinds[m, 1:] == D.FROZEN).nonzero().flatten()
        seen += frozen.numel()
        assert torch.equal(rows[:, frozen], rows[:1, frozen].expand(rows.shape[0], -1, -1)), f"{what}: clip {m}, dof_pos of a frozen joint changes between queries"
        assert (rows[:, frozen] != 0).any(dim=-1).all()
    assert seen > 0
    still = [c[2] for c in info["clips"]].index("still")
    s = int(tabs["length_starts"][still])
    rot = got["rb_rot"].cpu()[ids == still].view(torch.int32)
    assert rot.shape[0] >= 9 and torch.equal(rot, tabs["grs"][s:s + 1].view(torch.int32).expand_as(rot)), f"{what}: rb_rot of the still clip is not the stored grs"


# ------------------------------------------------------------------------------------------------ a. the query against the reference
def test_motion_state_matches_reference_fixture(dev):
    z, tabs, info = fixture()
    lib = MotionLib.from_tables(tabs, dev)
    ids, times, off = (torch.from_numpy(z[k]) for k in ("motion_ids", "motion_times", "offset"))
    cell_l, cell_g = D.cell_labels(tabs, info, ids, times)
    print(f"queried cells, lrs: {D.label_counts(cell_l)}\nqueried cells, grs: {D.label_counts(cell_g)}")
    assert all(c > 0 for c in D.label_counts(cell_l).values()) and all(c > 0 for c in D.label_counts(cell_g).values())
    want = {k: torch.from_numpy(z[k]) for k in EXACT + ROT}
    res = lib.get_motion_state(ids.to(dev), times.to(dev), off.to(dev))
    compare(res, want)
    kind_properties(tabs, info, ids, res, "with offset")
    fr = lib.query(ids.to(dev), times.to(dev), off.to(dev), with_frames=True)
    for k in ("frame_idx0", "frame_idx1", "blend"):
        assert torch.equal(fr[k].cpu(), torch.from_numpy(z[k])), k
    plain = lib.get_motion_state(ids.to(dev), times.to(dev))
    assert torch.equal(plain["rg_pos"].cpu(), torch.from_numpy(z["rg_pos_no_offset"]))
    compare(plain, want, keys_exact=("body_vel", "body_ang_vel", "dof_vel"))
    kind_properties(tabs, info, ids, plain, "without offset")
    assert torch.equal(lib.get_root_pos_smpl(ids.to(dev), times.to(dev))["root_pos"].cpu(), torch.from_numpy(z["root_pos_smpl"]))


# ------------------------------------------------------------------------------------------------ b. every lane form
@pytest.mark.parametrize("humanoid", ["smpl", 33, "smplx", 64])
def test_lane_forms_match_oracle_on_degenerate_clips(dev, humanoid):
    """24 bodies in the half-wave form (8 queries per workgroup), 33 / 52 / 64 in the whole-wave form (4 per workgroup); 381 queries = 4 x 95 + 1:
    the last workgroup is partial in both forms (5 of 8, 1 of 4)."""
    tabs, info, ids, times, off, want = library(humanoid)
    j = tabs["gts"].shape[1]
    lib = MotionLib.from_tables(tabs, dev)
    got = lib.query(ids.to(dev), times.to(dev), off.to(dev), with_frames=True, with_records=True)
    got["root_pos"], got["root_rot"], got["root_vel"], got["root_ang_vel"] = got["rg_pos"][:, 0], got["rb_rot"][:, 0], got["body_vel"][:, 0], got["body_ang_vel"][:, 0]
    assert got["rg_pos"].shape == (ids.numel(), j, 3) and got["dof_pos"].shape == (ids.numel(), 3 * (j - 1))
    compare(got, want)
    assert torch.equal(got["frame_idx0"].cpu() + tabs["length_starts"][ids], want["frame_idx0"])
    assert torch.equal(got["frame_idx1"].cpu() + tabs["length_starts"][ids], want["frame_idx1"]) and torch.equal(got["blend"].cpu(), want["blend"])
    assert torch.equal(got["rb_records"], torch.cat([got["rg_pos"], got["rb_rot"], got["body_vel"], got["body_ang_vel"]], dim=-1))
    kind_properties(tabs, info, ids, got, f"{j} bodies")


# ------------------------------------------------------------------------------------------------ c. query modes
def _envs(tabs, dev, ne=49):
    """Per-env inputs whose clock lands on t = 0, t = length and exact frame times of every clip, the 2- and 3-frame ones included."""
    m = tabs["motion_lengths"].shape[0]
    e = torch.arange(ne)
    ids = e % m
    g = syn.make_generator(SEED + 1)
    progress = torch.randint(0, 20, (ne,), generator=g)
    start = torch.rand(ne, generator=g) * 0.2
    start_off = (torch.rand(ne, generator=g) - 0.5) * 0.05
    progress[:2 * m] = e[:2 * m] // m                      # t = 0 and t = dt exactly on every clip (= length on the 2-frame clip at 30 fps) ...
    start[:3 * m], start_off[:3 * m] = 0.0, 0.0
    progress[2 * m:3 * m] = 0                              # ... and t = length exactly
    start[2 * m:3 * m] = tabs["motion_lengths"]
    off = torch.randn(ne, 3, generator=g)
    return {k: v.to(dev) for k, v in dict(ids=ids, progress=progress, start=start, start_off=start_off, off=off).items()}


def _times_mode(lib, ids, t, off=None):
    return lib.query(ids, t.contiguous(), off, with_frames=True, with_records=True)


def _same(got, want, keys, what):
    for k in keys:
        assert torch.equal(got[k], want[k]), (what, k)


@pytest.mark.parametrize("humanoid", ["smpl", "smplx"])
def test_clock_modes_equal_the_times_mode(dev, humanoid):
    tabs = library(humanoid)[0]
    lib = MotionLib.from_tables(tabs, dev)
    v = _envs(tabs, dev)
    ne, f32 = v["ids"].numel(), torch.float32
    dt = 1.0 / 30.0
    dt32 = torch.tensor(dt, dtype=f32, device=dev)
    length = lib._motion_lengths[v["ids"]]
    keys = FIELDS + ("frame_idx0", "frame_idx1", "blend")
    hit_zero = hit_len = 0
    for shift in (0, 1):
        t = (v["progress"] + shift).to(f32) * dt32
        t = t + v["start"]
        t = t + v["start_off"]
        hit_zero += int((t == 0).sum())
        hit_len += int((t == length).sum())
        got = lib.query(v["ids"], offset=v["off"], progress=v["progress"], step_shift=shift, dt=dt, start_times=v["start"], start_offsets=v["start_off"],
                        with_frames=True, with_records=True)
        _same(got, _times_mode(lib, v["ids"], t, v["off"]), keys, f"clock shift {shift}")
        # root_only: the root position alone, no offset (get_root_pos_smpl)
        root = lib.query(v["ids"], progress=v["progress"], step_shift=shift, dt=dt, start_times=v["start"], start_offsets=v["start_off"], root_only=True)
        assert torch.equal(root["root_pos"], _times_mode(lib, v["ids"], t)["rg_pos"][:, 0]), f"root_only shift {shift}"
    m = tabs["motion_lengths"].shape[0]
    assert hit_zero >= m and hit_len >= m                   # t = 0 and t = length exactly, on every clip
    # time_steps > 1: sample k of env e at ((progress + shift) dt + k traj_dt) + start + start_offset
    steps, traj_dt = 3, 1.0 / 30.0
    k = torch.arange(steps, device=dev).to(f32) * torch.tensor(traj_dt, dtype=f32, device=dev)
    t = ((v["progress"] + 1).to(f32) * dt32)[:, None] + k[None, :]
    t = t + v["start"][:, None]
    t = (t + v["start_off"][:, None]).reshape(-1)
    got = lib.query(v["ids"], offset=v["off"], progress=v["progress"], step_shift=1, dt=dt, start_times=v["start"], start_offsets=v["start_off"],
                    time_steps=steps, traj_dt=traj_dt, with_frames=True, with_records=True)
    assert got["rg_pos"].shape[0] == ne * steps
    _same(got, _times_mode(lib, v["ids"].repeat_interleave(steps), t, v["off"].repeat_interleave(steps, dim=0)), keys, "time_steps 3")


@pytest.mark.parametrize("time_interval", [False, True])
def test_reset_mode_at_phase_0_and_1_equals_the_times_mode(dev, time_interval):
    tabs = library("smpl")[0]
    lib = MotionLib.from_tables(tabs, dev)
    v = _envs(tabs, dev)
    ne, j, f32 = v["ids"].numel(), lib.num_bodies, torch.float32
    e = torch.arange(ne, device=dev)
    phase = torch.tensor([0.0, 1.0, 0.37], device=dev)[e % 3].contiguous()        # 8 clips x 3 phases: every combination within 24 envs
    mask = e % 5 != 0
    length = lib._motion_lengths[v["ids"]]
    st = phase * length
    if time_interval:                                                              # sample_time_interval, motion_lib_base.py:413-421
        c = torch.tensor(1.0 / 30.0, dtype=f32, device=dev)
        st = (st / c).long().to(f32) * c
    assert ((st == 0) & mask).sum() >= 8 and (time_interval or ((st == length) & mask).sum() >= 8)
    nan = float("nan")
    for zeroing in (False, True):
        out = {"rb_records": torch.full((ne, j, 13), nan, device=dev), "dof_pos": torch.full((ne, 3 * (j - 1)), nan, device=dev),
               "dof_vel": torch.full((ne, 3 * (j - 1)), nan, device=dev)}
        start_off, goff = v["start_off"].clone(), v["off"].clone()
        words = {"start_times": torch.full((ne,), nan, device=dev), "progress": torch.full((ne,), 7, dtype=torch.int64, device=dev),
                 "clear0": torch.full((ne,), 5, dtype=torch.int64, device=dev)}
        reset = dict(words, mask=mask, phase=phase, time_interval=time_interval)
        if zeroing:
            reset.update(zero_start_offsets=start_off, zero_global_offset=goff)
        lib.query(v["ids"], offset=goff, dt=1.0 / 30.0, start_offsets=start_off, out=out, fields=("rb_records", "dof_pos", "dof_vel"), reset=reset)
        want = _times_mode(lib, v["ids"], st if zeroing else st + v["start_off"], None if zeroing else v["off"])
        for k in out:
            assert torch.equal(out[k][mask], want[k][mask]), (zeroing, k)
            assert torch.isnan(out[k][~mask]).all(), (zeroing, k)
        assert torch.equal(words["start_times"][mask], st[mask]) and torch.isnan(words["start_times"][~mask]).all()
        assert (words["progress"][mask] == 0).all() and (words["progress"][~mask] == 7).all()
        assert (words["clear0"][mask] == 0).all() and (words["clear0"][~mask] == 5).all()
        if zeroing:
            assert (start_off[mask] == 0).all() and (goff[mask] == 0).all()
            assert torch.equal(start_off[~mask], v["start_off"][~mask]) and torch.equal(goff[~mask], v["off"][~mask])


@pytest.mark.parametrize("humanoid", ["smpl", "smplx"])
def test_rb_records_with_a_wider_pitch(dev, humanoid):
    from pulse_amd._lib import MotionStateArgs
    from pulse_amd._marshal import launch
    tabs, _, ids, times, off, _ = library(humanoid)
    lib = MotionLib.from_tables(tabs, dev)
    ids, times, off = ids.to(dev), times.to(dev), off.to(dev)
    n, j = ids.numel(), lib.num_bodies
    pitch = 13 * j + 7
    buf = torch.full((n, pitch), float("nan"), device=dev)
    a = MotionStateArgs()
    lib.fill_tables(a.tab)
    a.n, a.motion_ids, a.motion_times, a.offset = n, ids.data_ptr(), times.data_ptr(), off.data_ptr()
    a.rb_records, a.rb_query_stride = buf.data_ptr(), pitch
    launch("pulse_motion_state", ctypes.byref(a))
    want = _times_mode(lib, ids, times, off)["rb_records"]
    assert torch.equal(buf[:, :13 * j].reshape(n, j, 13), want) and torch.isnan(buf[:, 13 * j:]).all()


# ------------------------------------------------------------------------------------------------ d. AMP history from the motion
@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_golden_amp_variants", os.path.join(ROOT, "tools", "gen_golden_amp_variants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("version,subset", [(1, False), (2, True)])
def test_amp_hist_init_on_degenerate_clips(gen, dev, version, subset):
    """History frames at start - dt (k + 1): on exact frames walking back from t = length, below 0 on the short clips, inside the still
    stretch.  All 23 joints (the identity hands included) in version 1, the 19-joint subset in version 2."""
    _, tabs, info = fixture()
    lib = MotionLib.from_tables(tabs, dev)
    m, S, dt = tabs["motion_lengths"].shape[0], 6, 1.0 / 30.0
    what = [c[2] for c in D.CLIPS]
    ids = torch.arange(2 * m) % m
    starts = torch.cat([tabs["motion_lengths"], torch.tensor(dt, dtype=torch.float32) * torch.tensor([1.0, 1.3, 3.0, 5.5, 4.25, 7.0, 0.0, 2.6])])
    starts[m + what.index("stretch")] = 13.0 / 60.0       # 60 fps, frames 5 .. 9 still: the history reads t = 11/60, 9/60, 7/60, 5/60, 3/60
    k = S - 1
    times = (starts.unsqueeze(-1) + (-dt * (torch.arange(0, k) + 1))).view(-1)    # _init_amp_obs_ref, humanoid_amp.py:531-563
    assert torch.equal(times.view(-1, k), starts[:, None] + (torch.arange(k) + 1).float() * torch.tensor(-dt, dtype=torch.float32))   # the kernel's expression
    qi = ids.repeat_interleave(k)
    f0, f1, blend = OracleMotionLib(tabs)._frames(qi, times)
    local = f0 - tabs["length_starts"][qi]
    stretch = qi == what.index("stretch")
    assert (times < 0).sum() >= 8 and ((blend < 1e-4) | (blend > 1 - 1e-4)).sum() >= 20 and ((blend > 0.1) & (blend < 0.9)).sum() >= 5 and (stretch & (local >= D.STRETCH[0]) & (local < D.STRETCH[1])).sum() >= 3
    assert D.query_conditions(tabs, qi, times) == []
    mask = torch.ones(2 * m, dtype=torch.bool)
    mask[[3, 10]] = False
    W = AM.frame_width(version=version, has_dof_subset=subset)
    hist = torch.full((2 * m, S, W), float("nan"), device=dev)
    ops.amp_hist_init(lib, ids.to(dev), starts.to(dev), dt, mask.to(dev), hist, torch.tensor(gen.KEY, device=dev),
                      joint_ids=torch.tensor(gen.JOINTS19, dtype=torch.int32, device=dev) if subset else None, upright=True, version=version)
    twin = AM.AmpWindow(OracleMotionLib(tabs), ids, S, dt, gen.KEY, dof_subset=torch.tensor(gen.SUBSET) if subset else None, upright=True, version=version)
    want = torch.full((2 * m, S, W), float("nan"))
    want[:, 1:] = twin.motion_frames(qi, times).view(2 * m, k, W)
    want[~mask] = float("nan")
    np.testing.assert_allclose(hist.cpu().numpy(), want.numpy(), atol=1e-5, rtol=1e-5, equal_nan=True)


# ------------------------------------------------------------------------------------------------ e. the in-kernel reference of pulse_im_step
@pytest.mark.parametrize("humanoid", ["smpl", "smplx"])
def test_in_kernel_reference_equals_array_reference_on_degenerate_clips(dev, humanoid):
    """pulse_im_step blending its reference from the packed library == the same launch fed by pulse_motion_state's arrays, bit for bit
    (the pattern of test_in_kernel_reference_equals_array_reference, without an env around it)."""
    from pulse_amd._lib import PULSE_IM_RESET, PULSE_IM_REWARD, PULSE_IM_SELF_OBS, PULSE_IM_TASK_OBS
    tabs = library(humanoid)[0]
    lib = MotionLib.from_tables(tabs, dev)
    v = _envs(tabs, dev)
    n, j = v["ids"].numel(), lib.num_bodies
    g = syn.make_generator(SEED + 2)
    rb = syn.rigid_body_state(g, n, j).to(dev)
    dof_force, dof_vel = torch.randn(n, 3 * (j - 1), generator=g).to(dev), torch.randn(n, 3 * (j - 1), generator=g).to(dev)
    dt, traj_dt = 1.0 / 30.0, 1.0 / 30.0
    what = PULSE_IM_REWARD | PULSE_IM_RESET | PULSE_IM_SELF_OBS | PULSE_IM_TASK_OBS
    motion_len = lib._motion_lengths[v["ids"]].contiguous()
    common = dict(time_steps=2, dof_force=dof_force, dof_vel=dof_vel, cycle_counter=torch.zeros(n, dtype=torch.int64, device=dev),
                  track_ids=torch.arange(j, device=dev), reset_ids=torch.arange(j, device=dev), term_dist=torch.full((j,), 0.25, device=dev),
                  specs=dict(ops.DEFAULT_REWARD_SPECS), power_coef=0.0005, power_reward=True)
    # (a) arrays path: advance the clock by hand, query the library, feed the arrays
    prog = v["progress"] + 1
    t = prog * dt + v["start"] + v["start_off"]
    pass_time = t >= motion_len
    assert pass_time.any() and not pass_time.all()
    kw = dict(offset=v["off"], progress=prog, dt=dt, start_times=v["start"], start_offsets=v["start_off"])
    now = lib.query(v["ids"], step_shift=0, **kw)
    nxt = lib.query(v["ids"], step_shift=1, time_steps=2, traj_dt=traj_dt, **kw)
    ref = lambda r: {"pos": r["rg_pos"], "rot": r["rb_rot"], "vel": r["body_vel"], "ang": r["body_ang_vel"]}
    a = ops.im_step(rb, what=what, ref_now=ref(now), ref_next=ref(nxt), progress=prog, pass_time=pass_time, **common)
    # (b) fused path: clock and reference in-kernel
    progress_rw = v["progress"].clone()
    pass_out = torch.zeros(n, dtype=torch.bool, device=dev)
    track = {"rb": torch.full((n, j, 13), float("nan"), device=dev), "dof_pos": torch.full((n, 3 * (j - 1)), float("nan"), device=dev),
             "dof_vel": torch.full((n, 3 * (j - 1)), float("nan"), device=dev)}
    clock = {"progress_rw": progress_rw, "inc": 1, "dt": dt, "start_times": v["start"], "start_offsets": v["start_off"], "motion_len": motion_len,
             "cycle_motion": False, "max_episode_length": 300, "pass_time_out": pass_out}
    motion = {"lib": lib, "ids": v["ids"], "offset": v["off"], "traj_dt": traj_dt, "track_rb": track["rb"], "track_dof_pos": track["dof_pos"],
              "track_dof_vel": track["dof_vel"]}
    b = ops.im_step(rb, what=what, progress=progress_rw, clock=clock, motion=motion, **common)
    for k in ("obs", "rew", "rew_raw", "reset", "terminate"):
        assert torch.equal(a[k], b[k]), k
    assert torch.isfinite(b["obs"]).all() and torch.isfinite(b["rew"]).all()
    assert torch.equal(progress_rw, prog) and torch.equal(pass_out, pass_time)
    one = lib.query(v["ids"], step_shift=1, with_records=True, **kw)
    assert torch.equal(track["rb"], one["rb_records"]) and torch.equal(track["dof_pos"], one["dof_pos"]) and torch.equal(track["dof_vel"], one["dof_vel"])


# ------------------------------------------------------------------------------------------------ f. the tasks' reference-state reset
HSCALE, VSCALE = 0.1, 0.005


def _reset_inputs():
    if "reset" not in _shared:
        _, tabs, _ = fixture()
        m, n = tabs["motion_lengths"].shape[0], 25
        e = torch.arange(n)
        ids = e % m
        length = tabs["motion_lengths"][ids]
        times = torch.tensor([0.0, 1.0, 0.37])[e % 3] * length                     # phase 0, 1 and mid-clip: every (clip, phase) within 24 envs
        assert (times == 0).sum() >= 8 and (times == length).sum() >= 8
        lib = OracleMotionLib(tabs)
        assert D.query_conditions(tabs, ids, times) == []
        assert TM.heading_axis_xy(lib, ids, times).min() >= 0.1                    # input condition of the heading removal (tests/test_task_reset_gpu.py)
        hs, cp = syn.synthetic_height_field(), torch.cat([syn.center_height_points(), torch.zeros(9, 1)], dim=1)
        g = syn.make_generator(SEED + 3)
        draw = lambda: 3.0 + torch.rand(n, 2, generator=g) * torch.tensor([20.0, 24.0])
        xy = draw()
        root_rot = lib.get_motion_state(ids, times)["root_rot"]
        near = lambda xy: ((lambda c: (c - c.round()).abs() <= 1e-4 / HSCALE)(TM.center_sample_cells(torch.cat([xy, torch.zeros(n, 1), root_rot], dim=1), cp, HSCALE))).any(dim=-1).any(dim=-1)
        for _ in range(50):                                                        # no centre sample within 1e-4 m of a cell edge (there the device may take the neighbour)
            bad = near(xy)
            if not bad.any():
                break
            xy = torch.where(bad[:, None], draw(), xy)
        assert not near(xy).any()
        _shared["reset"] = (tabs, lib, ids, times, hs, cp, xy)
    return _shared["reset"]


@pytest.mark.parametrize("transform", ["none", "zero_xy", "remove_heading", "terrain"])
def test_task_ref_state_init_on_degenerate_clips(dev, transform):
    tabs, cpu_lib, ids, times, hs, cp, xy = _reset_inputs()
    n, j = ids.numel(), 24
    m = TM.ref_state(cpu_lib, ids, times, transform, upright=True, new_root_xy=xy, heightsamples=hs, center_points=cp, horizontal_scale=HSCALE,
                     vertical_scale=VSCALE)
    lib = MotionLib.from_tables(tabs, dev)
    kw = {"transform": transform, "upright": True}
    if transform == "terrain":
        kw.update(new_root_xy=xy.to(dev), heightsamples=hs.to(dev), horizontal_scale=HSCALE, vertical_scale=VSCALE, center_points=cp[:, :2].contiguous().to(dev))
    nan = float("nan")
    out = {"rb": torch.full((n, j, 13), nan, device=dev), "dof_pos": torch.full((n, 69), nan, device=dev), "dof_vel": torch.full((n, 69), nan, device=dev),
           "start_times": torch.full((n,), nan, device=dev), "sampled_ids": torch.full((n,), -7, dtype=torch.int64, device=dev)}
    mask = torch.arange(n) % 6 != 5
    ops.task_ref_state_init(lib, ids.to(dev), times.to(dev), mask.to(dev), out["rb"], out["dof_pos"], out["dof_vel"], out["start_times"], out["sampled_ids"], **kw)
    out = {k: t.cpu() for k, t in out.items()}
    for k in ("rb", "dof_pos", "dof_vel", "start_times"):
        assert torch.isnan(out[k][~mask]).all(), k
    assert (out["sampled_ids"][~mask] == -7).all()
    assert torch.equal(out["sampled_ids"][mask], ids[mask]) and torch.equal(out["start_times"][mask], times[mask])
    assert torch.equal(out["dof_vel"][mask], m["dof_vel"][mask])                   # a lerp, never transformed
    assert (out["dof_pos"][mask] - m["dof_pos"][mask]).abs().max().item() <= 2e-6
    got, want = out["rb"][mask], m["records"][mask]
    if transform == "none":
        for lo, hi in ((0, 3), (7, 10), (10, 13)):                                 # lerped: position, linear and angular velocity
            assert torch.equal(got[..., lo:hi], want[..., lo:hi]), lo
        assert (got[..., 3:7] - want[..., 3:7]).abs().max().item() <= 2e-6         # slerped
        return
    err = (got - want).abs().max().item()
    print(f"[degenerate task reset] {transform}: max abs error {err:.3e}")
    assert err <= 1e-5, err


# ------------------------------------------------------------------------------------------------ g. build, then query
# (query, dof joint) cells of the motion_build cases at which query_conditions does NOT hold: the local rotations of that fixture pass
# through w = 0 (a turn by pi, where the exp map jumps from +pi to -pi times the axis) on a few frames.  Every one of them has |w| < 1e-2;
# none is near the identity.  Their number on the reference's own tables, (cells, queries they sit in):
CLIFF_CELLS = {"still": (7, 7), "sign": (18, 13)}


def _reference_tables(z, name):
    nf = torch.from_numpy(z[f"{name}_frames"].astype(np.int64))
    fps = torch.from_numpy(z[f"{name}_fps"].astype(np.float64))
    tabs = {k: torch.from_numpy(z[f"{name}_{k}_expected"]) for k in MotionLib.FIELDS}
    tabs.update({"motion_num_frames": nf, "motion_fps": fps.float(), "motion_dt": (1.0 / fps).float(), "motion_lengths": ((1.0 / fps) * (nf - 1).double()).float(),
                 "length_starts": torch.cumsum(nf, 0) - nf})
    return tabs


@pytest.mark.parametrize("name", ["still", "sign"])
def test_built_records_query_like_the_oracle(dev, name):
    """pulse_motion_build writes the records, pulse_motion_state reads them: the still stretch (bit-identical inputs -> q0 branch) and the
    negated frames (-> flip) of tests/golden/motion_build.npz, built on the device, read back and queried at every query of
    degenerate_clips.queries -- every exact frame time, five times inside every blend, the clip edges.  Every query is asked and every
    field of it compared.  That fixture does not clear the |w| floor of query_conditions everywhere (CLIFF_CELLS): at exactly the
    (query, joint) cells query_conditions names -- the same on the reference's tables and on the built ones -- dof_pos is held to the
    oracle up to the sign the wrap at pi decides (2e-6 all the same), everywhere else as it stands."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "motion_build.npz"))
    rot, trans = z[f"{name}_rot"], torch.from_numpy(z[f"{name}_trans"])
    assert len(z[f"{name}_frames"]) == 1
    data = {"clip": {"pose_quat_global": rot, "root_trans_offset": trans, "fps": float(z[f"{name}_fps"][0])}}
    trees = (z[f"{name}_parents"].tolist(), torch.from_numpy(z[f"{name}_local_translation"]))
    lib = MotionLib.from_motion_data(data, trees, device=dev, im_eval=True)       # im_eval: no random heading, grs is the input
    tabs = lib.tables()
    assert torch.equal(tabs["grs"].view(torch.int32), torch.from_numpy(rot).view(torch.int32))
    assert D.unstable_pairs(tabs) == []                                            # still frames: identical bits; every other step of that fixture >= 0.02 rad
    lab = D.pair_labels(tabs)
    rows = lab["pair_rows"]
    counts = {k: D.label_counts(lab[k + "_labels"][rows]) for k in ("lrs", "grs")}
    print(f"{name}: {counts}")
    if name == "still":
        assert counts["lrs"]["q0"] >= 3 * 23 and counts["grs"]["q0"] >= 3 * 24                                        # frames 3 .. 6 still
    else:
        assert counts["grs"]["flip"] >= 2 * 24 and counts["lrs"]["flip"] >= 2                                         # frame 2 negated whole
    ref_tabs = _reference_tables(z, name)
    ids, times, off = D.queries(ref_tabs, SEED)
    cliff = D.query_conditions(ref_tabs, ids, times)
    cells = [(q, d) for q, d, _ in cliff]
    print(f"{name}: {len(ids)} queries, all asked; {len(cells)} (query, joint) cells in {len({q for q, _ in cells})} queries sit at the wrap of the exp map")
    assert (len(cells), len({q for q, _ in cells})) == CLIFF_CELLS[name] and all(abs(w) < D.MIN_ABS_W for _, _, w in cliff)
    assert [(q, d) for q, d, _ in D.query_conditions(tabs, ids, times)] == cells   # the built tables: the same cells, no other
    got = lib.query(ids.to(dev), times.to(dev), off.to(dev), with_frames=True)
    got["root_pos"], got["root_rot"], got["root_vel"], got["root_ang_vel"] = got["rg_pos"][:, 0], got["rb_rot"][:, 0], got["body_vel"][:, 0], got["body_ang_vel"][:, 0]
    want = OracleMotionLib(tabs).get_motion_state(ids, times, off)
    compare(got, want, keys_rot=("rb_rot", "root_rot"))
    for k in ("frame_idx0", "frame_idx1", "blend"):
        assert torch.equal(got[k].cpu(), want[k]), k                               # (one clip: length_starts is 0)
    n = ids.numel()
    g, w = got["dof_pos"].cpu().view(n, -1, 3), want["dof_pos"].view(n, -1, 3)
    at_wrap = torch.zeros(n, g.shape[1], dtype=torch.bool)
    at_wrap[[q for q, _ in cells], [d for _, d in cells]] = True
    assert (g - w)[~at_wrap].abs().max().item() <= 2e-6
    either = torch.minimum((g - w).abs().amax(dim=-1), (g + w).abs().amax(dim=-1))     # the whole exp map of a joint changes sign at the wrap
    assert either[at_wrap].max().item() <= 2e-6 and (w[at_wrap].norm(dim=-1) > 3.0).all()


# ------------------------------------------------------------------------------------------------ h. pulse_slerp on every pair
def test_slerp_op_on_every_consecutive_pair(dev):
    _, tabs, info = fixture()
    rows = np.nonzero(info["pair_rows"])[0]
    for k in ("lrs", "grs"):
        q0, q1 = tabs[k][rows].reshape(-1, 4), tabs[k][rows + 1].reshape(-1, 4)
        labels = torch.from_numpy(info[k + "_labels"][rows].reshape(-1))
        for t in (0.0, 0.25, 0.5, 1.0):
            tt = torch.full((q0.shape[0], 1), t)
            got = ops.slerp(q0.to(dev), q1.to(dev), tt.to(dev)).cpu()
            want = R.slerp(q0, q1, tt)
            err = (got - want).abs().max().item()
            assert err <= 5e-6, (k, t, err)
            same = (labels == D.Q0) | (labels == D.IDENT)                          # identical bits in, the same bits out on every branch
            assert torch.equal(got[same].view(torch.int32), q0[same].view(torch.int32)), (k, t)
            mid = labels % D.FLIP == D.MID
            assert (labels[mid] < D.FLIP).all()                                    # (a flipped midpoint pair would need -q1 below; the builder draws none)
            assert mid.any() and torch.equal(got[mid], 0.5 * q0[mid] + 0.5 * q1[mid]), (k, t)        # the fallback ignores t


# ------------------------------------------------------------------------------------------------ i. the grid-stride loop of rot_op_kernel
def test_rot_ops_past_one_grid(dev):
    """2048 blocks of 256 rows is the whole grid: 77 rows more take the loop's second trip (the largest m elsewhere in the suite is 98 304)."""
    m = 2048 * 256 + 77
    g = syn.make_generator(SEED + 4)
    q0 = torch.randn(m, 4, generator=g)
    q0 = q0 / q0.norm(dim=-1, keepdim=True)
    axis = torch.randn(m, 3, generator=g)
    h = 0.05 + 1.15 * torch.rand(m, 1, generator=g)                                # half-angle of the step: the general branch, |dot| >= cos 1.2 = 0.36
    dq = torch.cat([axis / axis.norm(dim=-1, keepdim=True) * torch.sin(h), torch.cos(h)], dim=-1)
    q1 = syn._quat_mul_xyzw(dq, q0)
    q1 = q1 / q1.norm(dim=-1, keepdim=True) * torch.where(torch.rand(m, 1, generator=g) < 0.5, -1.0, 1.0)
    t = torch.rand(m, 1, generator=g)
    rows = torch.cat([torch.arange(0, m - 77, 997), torch.arange(m - 77, m)])
    stable, label = D.classify(q0[rows].numpy(), q1[rows].numpy())
    assert stable.all() and (label % D.FLIP == D.GEN).all() and (label >= D.FLIP).any() and (label < D.FLIP).any()
    got_mul = ops.quat_mul(q0.to(dev), q1.to(dev))[rows.to(dev)].cpu()
    got_slerp = ops.slerp(q0.to(dev), q1.to(dev), t.to(dev))[rows.to(dev)].cpu()
    assert (got_mul - R.qmul(q0[rows], q1[rows])).abs().max().item() <= 2e-6
    assert (got_slerp - R.slerp(q0[rows], q1[rows], t[rows])).abs().max().item() <= 5e-6
