"""GPU: pulse_task_step, pulse_traj_step and pulse_traj_generate against the CPU oracle (oracle/task_oracle.py) on the paths the golden
tests leave out: more than one workgroup and a ragged last one, the env_ids / env_mask subsets, sensor grids that straddle or leave the
height field, grids of 20 x 20 and 33 x 33 points, heights relative to the root's z, the root as sensor body, exact vertex times and
the phase clamp of the trajectory table, fuzzy_target, disable_collision and the power term at 153 dofs.  The oracle is pinned to the
reference on these inputs by tests/test_task_edges_oracle.py; the inputs are built by tests/task_edge_cases.py.

Floats: 1e-5 absolute + 1e-5 relative (observations, O(1) rewards), 1e-5 of the largest magnitude (power term), 2e-5 (generated
vertices).  Flags bit for bit, after the fp64 check that no input sits within 1e-3 of a decision threshold."""
import numpy as np
import pytest
import torch

import task_edge_cases as C
from oracle import task_oracle as TO
from pulse_amd import ops, synthetic as syn
from pulse_amd._lib import TASK_OBS, TASK_RESET, TASK_REWARD
from test_terrain_gpu import Z as ZTERRAIN, explain_height_differences

pytestmark = pytest.mark.gpu
ALL = TASK_OBS | TASK_REWARD | TASK_RESET
POISON = -777.25


def close(got, want, what=""):
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.numpy(), atol=1e-5, rtol=1e-5, err_msg=what)


def same_flags(got, want, what=""):
    assert torch.equal(got.cpu(), want), what


@pytest.fixture(scope="module")
def tasks(dev):
    d = C.task_inputs()
    C.task_margins(d)
    return d, C.task_expected(d), {k: v.to(dev) for k, v in d.items() if isinstance(v, torch.Tensor)}


@pytest.fixture(scope="module")
def scene(dev):
    s = C.terrain_scene()
    tar64 = TO.traj_calc_pos(s["verts"].double(), torch.arange(s["n"]), s["progress"].double() * C.STEP_DT, s["traj_dt"])
    C.traj_margins(s["rb"], tar64, s["contact"], C.FAIL_DIST)
    s["tar"] = TO.traj_calc_pos(s["verts"], torch.arange(s["n"]), s["progress"] * C.STEP_DT, s["traj_dt"])
    return s, {k: v.to(dev) for k, v in s.items() if isinstance(v, torch.Tensor)}


def _task_kw(task, g, power=None):
    """The keyword arguments of one full ops.task_step launch (observation, reward and reset) of ``task``."""
    kw = dict(what=ALL, dt=1.0 / 30.0, contact_forces=g["contact"], contact_body_ids=C.CONTACT_IDS, termination_heights=g["term_h"],
              progress=g["progress"], max_episode_length=300.0)
    if task == "speed":
        kw.update(prev_root_pos=g["prev_root_pos"], tar_speed=g["tar_speed"])
    elif task == "reach":
        kw.update(tar_pos=g["tar_pos"], reach_body_id=23)
    else:
        kw.update(prev_root_pos=g["prev_root_pos"], tar_states=g["tar_states"], tar_contact_forces=g["tar_contact"], strike_body_ids=C.STRIKE_IDS)
    if power is not None:
        kw.update(dof_force=power[0], dof_vel=power[1], power_reward=True)
    return kw


# ---------------------------------------------------------------------------------------------------------------------
# 1. pulse_task_step over two workgroups (256 + 44 envs)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", ["speed", "reach", "strike"])
def test_task_step_two_blocks_vs_oracle(tasks, task):
    d, want, g = tasks
    n = d["n"]
    assert n == 300 and all(o // 256 == b for b, o in enumerate(C.CASE_BLOCKS))
    out = ops.task_step(task, g["rb"], **_task_kw(task, g))
    close(out["obs"], want[f"{task}_obs"], "obs")
    close(out["rew"], want[f"{task}_rew"], "rew")
    close(out["rew_raw"][:, 0], want[f"{task}_rew"], "rew_raw")
    tag = "strike_" if task == "strike" else ""
    same_flags(out["reset"], want[f"{tag}reset"], "reset")
    same_flags(out["terminate"], want[f"{tag}terminated"], "terminate")
    out = ops.task_step(task, g["rb"], **{**_task_kw(task, g), "what": TASK_RESET, "enable_early_termination": False})
    same_flags(out["reset"], want["reset_noearly"])
    assert (out["terminate"] == 0).all()
    # the deliberate cases do what they were placed for, in both blocks
    for o in C.CASE_BLOCKS:
        assert want["terminated"][o + 12:o + 22].tolist() == [0, 0, 1, 0, 0, 0, 0, 1, 0, 0]
        assert want["strike_terminated"][o + 12:o + 22].tolist() == [0, 0, 1, 0, 0, 0, 0, 1, 1, 0]
        assert want["reset"][o + 12:o + 22].tolist() == [0, 0, 1, 0, 1, 1, 0, 1, 0, 0]
        assert (want["strike_rew"][o + 5:o + 10] == 1.0).all() and (want["strike_rew"][o:o + 5] < 1.0).all()
        assert (C._strike_scalars(d, torch.float64)[1][o + 10:o + 12] < 0).all()
    assert 0 < want["terminated"][256:].sum() < 44 and not torch.equal(want["terminated"], want["strike_terminated"])


# ---------------------------------------------------------------------------------------------------------------------
# 2. env_ids / env_mask / both
# ---------------------------------------------------------------------------------------------------------------------
def _subsets(n, ids, dev, seed):
    """(name, env_ids, env_mask, selected) for the three subset forms; ``ids`` unordered, the last env among them."""
    mask = torch.rand(n, generator=syn.make_generator(seed)) < 0.4
    mask[n - 1], mask[ids[1]] = True, False
    ids = torch.tensor(ids)
    by_ids = torch.zeros(n, dtype=torch.bool)
    by_ids[ids] = True
    assert ids[0] == n - 1 and (by_ids & mask).any() and (by_ids & ~mask).any() and (mask & ~by_ids).any()
    return (("env_ids", ids.to(dev), None, by_ids), ("env_mask", None, mask.to(dev), mask), ("env_ids + env_mask", ids.to(dev), mask.to(dev), by_ids & mask))


def _poisoned(n, width, dev):
    return {"obs": torch.full((n, width), POISON, device=dev), "rew": torch.full((n,), POISON, device=dev),
            "rew_raw": torch.full((n, 2), POISON, device=dev), "reset": torch.full((n,), -7, dtype=torch.int64, device=dev),
            "terminate": torch.full((n,), -7, dtype=torch.int64, device=dev)}


def _check_subset(name, out, full, sel, off, w):
    sel = sel.to(out["obs"].device)
    assert (out["obs"][:, :off] == POISON).all() and (out["obs"][:, off + w:] == POISON).all(), name   # the columns around the task block
    for k, poison in (("obs", POISON), ("rew", POISON), ("rew_raw", POISON), ("reset", -7), ("terminate", -7)):
        got = out[k][:, off:off + w] if k == "obs" else out[k]
        ref = full[k][:, off:off + w] if k == "obs" else full[k]
        assert torch.equal(got[sel], ref[sel]), (name, k)
        assert (got[~sel] == poison).all(), (name, k, "a row outside the subset was written")
        assert not (ref[sel] == poison).any()


@pytest.mark.parametrize("task", ["speed", "reach", "strike"])
def test_task_step_subsets_leave_other_rows_alone(dev, tasks, task):
    d, _, g = tasks
    n, off, w = d["n"], 358, {"speed": 3, "reach": 3, "strike": 15}[task]
    power = [t.to(dev) for t in C.power_inputs(n, 69)[:2]]
    kw = _task_kw(task, g, power)
    full = _poisoned(n, 384, dev)
    ops.task_step(task, g["rb"], obs_offset=off, **full, **kw)
    for name, ids, mask, sel in _subsets(n, [299, 3, 270, 255, 256, 17, 130, 0, 298], dev, 21):
        out = _poisoned(n, 384, dev)
        ops.task_step(task, g["rb"], obs_offset=off, env_ids=ids, env_mask=mask, **out, **kw)
        _check_subset(name, out, full, sel, off, w)


def _scene_kw(s, g, dev, num_dof=69):
    df, dv, _ = C.power_inputs(s["n"], num_dof)
    return dict(what=ALL, dt=C.STEP_DT, episode_dur=C.EPISODE_DUR, heightsamples=g["hs"], height_points=syn.square_height_points(2.0, 20).to(dev),
                center_points=syn.center_height_points().to(dev), sensor_body=C.HEAD, use_center_height=True, dof_force=df.to(dev), dof_vel=dv.to(dev),
                power_reward=True, contact_forces=g["contact"], contact_body_ids=C.CONTACT_IDS, termination_heights=g["term_h"], fail_dist=C.FAIL_DIST)


def test_traj_step_subsets_leave_other_rows_alone(dev, scene):
    s, g = scene
    n, off, w = s["n"], 8, 20 + 400
    kw = _scene_kw(s, g, dev)
    full = _poisoned(n, off + w + 4, dev)
    ops.traj_step(g["rb"], g["verts"], g["progress"], obs_offset=off, **full, **kw)
    for name, ids, mask, sel in _subsets(n, [47, 3, 30, 12, 0, 46, 21], dev, 22):
        out = _poisoned(n, off + w + 4, dev)
        ops.traj_step(g["rb"], g["verts"], g["progress"], obs_offset=off, env_ids=ids, env_mask=mask, **out, **kw)
        _check_subset(name, out, full, sel, off, w)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the power term at 69 and 153 dofs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_dof", [69, 153])
def test_power_term_row_sums(dev, tasks, scene, num_dof):
    d, want, g = tasks
    n = d["n"]
    df, dv, pw = C.power_inputs(n, num_dof)
    progress = torch.arange(n) % 8                                            # both sides of the ``progress <= 3`` gate, in both blocks
    pw_t = torch.where(progress <= 3, torch.zeros_like(pw), pw)
    out = ops.task_step("speed", g["rb"], what=TASK_REWARD, prev_root_pos=g["prev_root_pos"], dt=d["dt"], tar_speed=g["tar_speed"], dof_force=df.to(dev),
                        dof_vel=dv.to(dev), progress=progress.to(dev), power_reward=True)
    assert (out["rew_raw"][:, 1].cpu().double() - pw_t).abs().max().item() <= 1e-5 * pw.abs().max().item()
    assert (out["rew_raw"][progress.to(dev) <= 3, 1] == 0).all() and (pw_t[256:] != 0).sum() > 10
    close(out["rew_raw"][:, 0], want["speed_rew"])
    close(out["rew"], (want["speed_rew"].double() + pw_t).float())
    s, gs = scene
    df, dv, pw = C.power_inputs(s["n"], num_dof)
    loc = TO.location_reward(s["rb"][:, 0, 0:3], s["tar"])
    kw = dict(what=TASK_REWARD, dt=C.STEP_DT, episode_dur=C.EPISODE_DUR, dof_force=df.to(dev), dof_vel=dv.to(dev))
    out = ops.traj_step(gs["rb"], gs["verts"], gs["progress"], power_reward=True, **kw)
    assert (out["rew_raw"][:, 1].cpu().double() - pw).abs().max().item() <= 1e-5 * pw.abs().max().item()
    close(out["rew_raw"][:, 0], loc)
    close(out["rew"], (loc.double() + pw).float())
    out = ops.traj_step(gs["rb"], gs["verts"], gs["progress"], power_reward=False, **kw)
    close(out["rew"], loc)
    assert (out["rew_raw"][:, 1].cpu().double() - pw).abs().max().item() <= 1e-5 * pw.abs().max().item()


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. the height map at the borders of the field, for grids that do not fill a pass of 4 x 256 points
# ---------------------------------------------------------------------------------------------------------------------
HEIGHT_CASES = [  # (grid resolution, use_center_height, sensor body, upright): every value at least twice, 33 x 33 with both centre settings
    (20, True, "head", True), (20, False, "root", False), (32, False, "head", False), (32, True, "root", True),
    (33, True, "root", False), (33, False, "head", True), (33, True, "head", False), (33, False, "root", True)]


@pytest.mark.parametrize("res,center,sensor,upright", HEIGHT_CASES)
def test_height_map_at_map_edges_and_grid_sizes(dev, scene, res, center, sensor, upright):
    s, g = scene
    n, rb, hs = s["n"], s["rb"], s["hs"]
    body = C.HEAD if sensor == "head" else 0
    hp, cp = syn.square_height_points(2.0, res), syn.center_height_points()
    nh, off = res * res, 12
    # conditions on the placement, by the reference's arithmetic alone: few samples can flip, none of the centre points can, and the
    # samples are a real mix of clipped and unclipped ones
    pts = C.sensor_points(rb, hp, body, upright)
    share = C.on_edge(pts).float().mean().item()
    un = C.unclipped(pts)
    partial = int(((un.sum(1) > 0) & (un.sum(1) < nh)).sum())
    print(f"[edges] grid {res}x{res} center={center} sensor={sensor} upright={upright}: {share:.2e} of the samples lie within 8 ulps of a cell edge; "
          f"{un.float().mean().item():.3f} unclipped, {partial} of {n} envs partially clipped")
    assert share <= 2e-3
    assert not C.on_edge(C.center_points_world(rb, cp, upright)).any()
    assert un.float().mean().item() >= 0.25 and (~un).float().mean().item() >= 0.25 and partial >= n // 2
    cells = (pts[..., :2] / C.HSCALE).long()
    for axis, size in ((0, C.MAP_ROWS), (1, C.MAP_COLS)):                     # each clip of each axis acts on hundreds of samples
        assert (cells[..., axis] < 0).sum() > 500 and (cells[..., axis] > size - 2).sum() > 500
    samples = TO.fetch_traj_samples(s["verts"], s["progress"], C.STEP_DT, s["traj_dt"], 10, 0.5)
    want = TO.terrain_task_obs(rb[:, 0], rb[:, body, 0:7], samples, hs, C.pad3(hp), C.pad3(cp), upright=upright, use_center_height=center)
    obs = torch.full((n, off + 20 + nh + 3), float("nan"), device=dev)
    ops.traj_step(g["rb"], g["verts"], g["progress"], what=TASK_OBS, dt=C.STEP_DT, episode_dur=C.EPISODE_DUR, upright=upright, heightsamples=g["hs"],
                  height_points=hp.to(dev), center_points=cp.to(dev) if center else None, sensor_body=body, use_center_height=center, obs=obs,
                  obs_offset=off)
    got = obs[:, off:off + 20 + nh].cpu()
    assert torch.isnan(obs[:, :off]).all() and torch.isnan(obs[:, off + 20 + nh:]).all() and not torch.isnan(got).any()
    close(got[:, :20], want[:, :20], "trajectory samples")
    flips = explain_height_differences(got[:, 20:], want[:, 20:], rb, upright, hs=hs, hp=hp, cp=cp, sensor_body=body, use_center_height=center)
    print(f"[edges] {flips} of {n * nh} height samples sit on a cell edge and take the neighbouring cell")
    assert flips <= 2e-3 * n * nh


# ---------------------------------------------------------------------------------------------------------------------
# 6. trajectory time: exact vertices, between them, past the end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_samples,upright", [(1, True), (10, False), (16, True)])
def test_trajectory_time_on_vertices_between_and_past_the_end(dev, num_samples, upright):
    """Five vertices, episode_dur 6.4, dt 0.5: the table lasts 5 x 1.6 = 8 s, so a sample at time t has the segment coordinate t / 2, exact in
    fp32 for every multiple of 0.25 s.  progress 0, 4 .. 16 land on the vertices, odd ones between them, 17 and more past the end."""
    nv, episode_dur, dt, step = 5, 6.4, 0.5, 0.75
    traj_dt = episode_dur / (nv - 1)
    assert np.float32(nv * traj_dt) == 8.0
    progress = torch.tensor([0, 4, 8, 12, 16, 1, 3, 5, 7, 9, 15, 17, 20, 40, 2, 6, 11, 13])
    n = progress.numel()
    g = syn.make_generator(31)
    rb = syn.rigid_body_state(g, n)
    verts = torch.zeros(n, nv, 3)
    verts[..., 0:2] = rb[:, None, 0, 0:2] + 1.5 * torch.randn(n, nv, 2, generator=g)
    verts[13, 4, 0:2] = rb[13, 0, 0:2] + 0.3                                  # progress 40: a time-out next to its target, not a failure
    seg = (progress.double() * dt).clamp(max=8.0) / 2
    assert (seg[:5] == torch.arange(5)).all() and (seg[11:14] == 4).all() and ((seg[5:11] % 1) != 0).all()
    samples = TO.fetch_traj_samples(verts, progress, dt, traj_dt, num_samples, step)
    assert torch.equal(samples[:5, 0], verts[torch.arange(5), torch.arange(5)])                     # the first sample IS the vertex
    assert torch.equal(samples[11:14], verts[11:14, None, 4].expand(-1, num_samples, -1))           # every sample clamped to the last vertex
    tar = TO.traj_calc_pos(verts, torch.arange(n), progress * dt, traj_dt)
    contact, term_h, fail = torch.zeros(n, 24, 3), torch.full((24,), C.TERM_H), 2.0
    C.traj_margins(rb, TO.traj_calc_pos(verts.double(), torch.arange(n), progress.double() * dt, traj_dt), contact, fail)
    want_reset = TO.traj_reset(torch.zeros(n, dtype=torch.long), progress, contact, C.CONTACT_IDS, rb[..., 0:3].contiguous(), tar, 21.0, fail, True, term_h)
    assert 0 < want_reset[1].sum() < n and (want_reset[0] != want_reset[1]).any()
    out = ops.traj_step(rb.to(dev), verts.to(dev), progress.to(dev), what=ALL, dt=dt, episode_dur=episode_dur, num_samples=num_samples,
                        sample_timestep=step, upright=upright, contact_forces=contact.to(dev), contact_body_ids=C.CONTACT_IDS,
                        termination_heights=term_h.to(dev), max_episode_length=21.0, fail_dist=fail, terrain_reset=False)
    assert out["obs"].shape[1] >= 2 * num_samples
    close(out["obs"][:, :2 * num_samples], TO.traj_location_observations(rb[:, 0], samples, upright), "trajectory samples")
    close(out["rew"], TO.location_reward(rb[:, 0, 0:3], tar), "reward")
    same_flags(out["reset"], want_reset[0])
    same_flags(out["terminate"], want_reset[1])


# ---------------------------------------------------------------------------------------------------------------------
# 7. fuzzy_target
# ---------------------------------------------------------------------------------------------------------------------
def test_fuzzy_target_reward(dev):
    t = lambda k: torch.from_numpy(ZTERRAIN[k])
    # the reference's golden (compute_location_reward_fuzzy on tar_pos + 0.03) through two-vertex tables that hold the target
    root, tar = t("rb")[:, 0], t("tar_pos") + 0.03
    err64 = ((tar[:, 0:2].double() - root[:, 0:2].double()) ** 2).sum(-1)
    C.assert_off(err64, 0.0025, "squared distance to the target")
    kw = dict(what=TASK_REWARD, dt=float(ZTERRAIN["dt"]), episode_dur=10.0)
    out = ops.traj_step(t("rb").to(dev), tar[:, None, :].repeat(1, 2, 1).contiguous().to(dev), torch.zeros(root.shape[0], dtype=torch.long, device=dev),
                        fuzzy_target=True, **kw)
    close(out["rew"], t("loc_rew_fuzzy"), "golden loc_rew_fuzzy")
    # envs on both sides of the 0.0025 threshold
    err = torch.tensor([0.0, 1e-4, 5e-4, 1e-3, 2e-3, 2.4e-3, 2.49e-3, 2.51e-3, 2.6e-3, 3e-3, 5e-3, 1e-2, 0.1, 1.0])
    n = err.numel()
    g = syn.make_generator(41)
    rb = syn.rigid_body_state(g, n)
    ang = 6.2831853 * torch.rand(n, generator=g)
    tar = rb[:, 0, 0:3].clone()
    tar[:, 0:2] += err.sqrt()[:, None] * torch.stack([ang.cos(), ang.sin()], 1)
    verts = tar[:, None, :].repeat(1, 2, 1).contiguous()
    progress = torch.randint(0, 300, (n,), generator=g)
    at = lambda v, p: TO.traj_calc_pos(v, torch.arange(n), p * kw["dt"], 10.0)
    err64 = ((at(verts.double(), progress.double())[:, 0:2] - rb[:, 0, 0:2].double()) ** 2).sum(-1)
    C.assert_off(err64, 0.0025, "squared distance to the target")
    inside = err64 < 0.0025
    assert inside.tolist() == [True] * 7 + [False] * 7
    fuzzy, plain = TO.location_reward(rb[:, 0, 0:3], at(verts, progress), fuzzy=True), TO.location_reward(rb[:, 0, 0:3], at(verts, progress))
    a = ops.traj_step(rb.to(dev), verts.to(dev), progress.to(dev), fuzzy_target=True, **kw)
    b = ops.traj_step(rb.to(dev), verts.to(dev), progress.to(dev), fuzzy_target=False, **kw)
    close(a["rew"], fuzzy, "fuzzy")
    close(b["rew"], plain, "plain")
    assert (a["rew"].cpu()[inside] == 1.0).all() and (b["rew"].cpu()[inside][1:] < 1.0).all()
    assert torch.equal(a["rew"].cpu()[~inside], b["rew"].cpu()[~inside]) and torch.equal(a["rew_raw"][:, 0], a["rew"])


# ---------------------------------------------------------------------------------------------------------------------
# 8. disable_collision (the reference's flags.no_collision_check; terrain variant only, see test_task_edges_oracle.py)
# ---------------------------------------------------------------------------------------------------------------------
def test_disable_collision_clears_failures_of_the_terrain_reset(dev, scene):
    s, g = scene
    n, z0, bp = s["n"], torch.zeros(s["n"], dtype=torch.long), s["rb"][..., 0:3].contiguous()
    kw = dict(what=TASK_RESET, dt=C.STEP_DT, episode_dur=C.EPISODE_DUR, contact_forces=g["contact"], contact_body_ids=C.CONTACT_IDS,
              termination_heights=g["term_h"], fail_dist=C.FAIL_DIST)
    for terrain, disable in ((True, False), (True, True), (False, False)):
        if terrain:
            want = TO.terrain_reset(z0, s["progress"], s["contact"], C.CONTACT_IDS, bp, s["tar"], 300.0, C.FAIL_DIST, True, disable_collision=disable)
        else:
            want = TO.traj_reset(z0, s["progress"], s["contact"], C.CONTACT_IDS, bp, s["tar"], 300.0, C.FAIL_DIST, True, s["term_h"])
        out = ops.traj_step(g["rb"], g["verts"], g["progress"], terrain_reset=terrain, disable_collision=disable, **kw)
        same_flags(out["reset"], want[0], (terrain, disable))
        same_flags(out["terminate"], want[1], (terrain, disable))
        if disable:
            assert want[1].sum() == 0 and torch.equal(want[0], (s["progress"] >= 299).long()) and want[0].sum() > 0
        else:
            assert 0 < want[1].sum() < n
    on = TO.terrain_reset(z0, s["progress"], s["contact"], C.CONTACT_IDS, bp, s["tar"], 300.0, C.FAIL_DIST, True)
    off = TO.traj_reset(z0, s["progress"], s["contact"], C.CONTACT_IDS, bp, s["tar"], 300.0, C.FAIL_DIST, True, s["term_h"])
    assert not torch.equal(on[1], off[1])                                    # the two variants differ on these inputs


# ---------------------------------------------------------------------------------------------------------------------
# 9. pulse_traj_generate over three workgroups (64 + 64 + 2 envs)
# ---------------------------------------------------------------------------------------------------------------------
def test_traj_generate_three_blocks_vs_oracle(dev):
    n, nv = 130, C.NUM_VERTS
    g = syn.make_generator(51)
    rb = syn.rigid_body_state(g, n)
    rb[:, :, 0:2] += 12.0 + 6.0 * torch.rand(n, 1, 2, generator=g)
    u = C.traj_draws(n, nv, 52)
    want = C.verts_from_draws(rb[:, 0, 0:3], u, C.EPISODE_DUR / (nv - 1))
    ud = {k: v.to(dev) for k, v in u.items()}
    args = (ud["dtheta"], ud["sharp"], ud["sharp_mask"], ud["heading"], ud["dspeed"], ud["speed0"])
    assert u["sharp_mask"].any() and u["sharp_mask"][64:].any()
    verts = torch.full((n, nv, 3), float("nan"), device=dev)
    ops.traj_generate(rb.to(dev), verts, *args, episode_dur=C.EPISODE_DUR)
    err = (verts.cpu() - want).abs().amax(dim=(1, 2))
    print(f"[traj_generate] largest vertex error per block: {err[:64].max().item():.2e} {err[64:128].max().item():.2e} {err[128:].max().item():.2e}")
    assert not torch.isnan(verts).any() and err.max().item() <= 2e-5
    mask = torch.zeros(n, dtype=torch.bool)
    mask[::3] = True
    assert mask[:64].any() and mask[64:128].any() and mask[128:].any() and not mask[128:].all()
    v2 = torch.full((n, nv, 3), POISON, device=dev)
    ops.traj_generate(rb.to(dev), v2, *args, episode_dur=C.EPISODE_DUR, env_mask=mask.to(dev))
    assert torch.equal(v2[mask.to(dev)], verts[mask.to(dev)]) and (v2[~mask.to(dev)] == POISON).all()
