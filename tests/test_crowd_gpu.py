"""GPU: the crowd kernels (pulse_amd/csrc/crowd_obs.hip: pulse_crowd_group_obs, pulse_crowd_stamp, pulse_crowd_heights) and
HumanoidPedestrianTerrain(Z) in its crowd / velocity modes, against the reference's recorded outputs (tests/golden/crowd.npz) and the CPU
model held bit for bit to them (tests/crowd_model.py, tests/test_crowd_cpu.py).

Tolerance: floats 1e-5 absolute, the standing tolerance for env observations (header of test_terrain_gpu.py); cell lists, owner grids and
resets exact.  The scenes keep every sample point and root point more than 2e-4 cells (13 fp32 ulps) from a cell edge and every distance
gap above 1e-4 relative (asserted on the committed arrays in test_crowd_cpu.py), so a device heading that differs from libm's by an ulp
cannot move a point into another cell or reorder neighbours: heights and stamps must agree as indices, and no edge allowance is made.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import crowd_model as M
from pulse_amd import _lib, configs, ops, synthetic as syn

pytestmark = pytest.mark.gpu
Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "crowd.npz"))
HS = syn.synthetic_height_field()
CP = syn.center_height_points()
CASES = M.golden_cases(Z)
SCENES = [M.scene_name(n, g) for n, g in M.SHAPES]
TOL = 1e-5
_model = {}


def model(c):
    """The model's block for every env of a golden case, computed once and shared."""
    if c["key"] not in _model:
        _model[c["key"]] = M.model_case(c, HS)
    return _model[c["key"]]


def run_kernels(c, dev, rb=None, env_ids=None, env_mask=None, fill=float("nan")):
    """[height block | people block] of one case through the C ABI wrappers, into a NaN-filled buffer at a column offset (as the env does)."""
    rb = (c["rb"] if rb is None else rb).to(dev)
    n, g, kind = rb.shape[0], c["group_size"], c["kind"]
    hp = syn.square_height_points(2.0, c["res"]).to(dev)
    stamps, vel = kind in ("stamps", "stamps_velocity"), kind in ("stamps_velocity", "velocity")
    hw = hp.shape[0] * (3 if vel else 1)
    width = hw + (M.GROUP_OBS if kind == "group_obs" else 0)
    off = 6                                                                                # an unaligned column offset
    obs = torch.full((n, off + width + 5), fill, device=dev)
    owner = None
    if stamps:
        owner = torch.zeros(n // g, *HS.shape, dtype=torch.int32, device=dev)
        cells = torch.full((n, M.ROOT_POINTS), -1, dtype=torch.int32, device=dev)
        ops.crowd_stamp(rb, g, owner, cells)
    sel = dict(env_ids=None if env_ids is None else env_ids.to(dev), env_mask=None if env_mask is None else env_mask.to(dev))
    if stamps or vel:
        ops.crowd_heights(rb, HS.to(dev), hp, group_size=g, owner=owner, velocity_map=vel, upright=c["upright"], sensor_body=c["sensor_body"],
                          center_points=CP.to(dev), use_center_height=c["center"], obs=obs, obs_offset=off, **sel)
    else:                                                                                  # group_obs: the plain heights are pulse_traj_step's
        ops.crowd_heights(rb, HS.to(dev), hp, upright=c["upright"], sensor_body=c["sensor_body"], center_points=CP.to(dev),
                          use_center_height=c["center"], obs=obs, obs_offset=off, **sel)
        ops.crowd_group_obs(rb, g, upright=c["upright"], obs=obs, obs_offset=off + hw, **sel)
    torch.cuda.synchronize()
    out = obs.cpu()
    assert torch.isnan(out[:, :off]).all() and torch.isnan(out[:, off + width:]).all()      # nothing outside the block is written
    return out[:, off:off + width]


@pytest.mark.parametrize("scene", SCENES + ["overlap", "res32"])
def test_kernels_match_the_reference_and_the_model(dev, scene):
    cases = [c for c in CASES if c["scene"] == scene]
    assert cases
    for c in cases:
        got = run_kernels(c, dev)
        assert torch.isfinite(got).all(), c["key"]
        d_ref = (got[c["rows"]] - c["ref"]).abs().max().item()
        d_mod = (got - model(c)).abs().max().item()
        print(f"[crowd] {c['key']}: max |kernel - reference| {d_ref:.3g} on {len(c['rows'])} envs, max |kernel - model| {d_mod:.3g} on {got.shape[0]}")
        assert d_ref <= TOL and d_mod <= TOL, c["key"]
        if c["kind"] == "group_obs":                                                        # zeroed neighbours are exact zeros
            want = model(c)[:, -M.GROUP_OBS:]
            assert torch.equal(got[:, -M.GROUP_OBS:] == 0, want == 0), c["key"]


@pytest.mark.parametrize("scene", SCENES)
def test_env_mask_and_env_ids_write_only_their_rows(dev, scene):
    """Subsets that cut through groups: unselected rows stay NaN, selected rows still see every neighbour and every stamp."""
    for kind in M.KINDS:
        c = next(c for c in CASES if c["scene"] == scene and c["kind"] == kind)
        n = c["rb"].shape[0]
        rows = torch.from_numpy(Z[f"{scene}/rows"])
        if len(rows) == n:
            rows = rows[1::3]
        mask = torch.zeros(n, dtype=torch.bool)
        mask[rows] = True
        ids = rows.flip(0)                                                                  # an id list in another order
        for sel in (dict(env_mask=mask), dict(env_ids=ids), dict(env_ids=torch.arange(n), env_mask=mask)):
            got = run_kernels(c, dev, **sel)
            assert torch.isnan(got[~mask]).all(), (c["key"], list(sel))
            assert (got[mask] - model(c)[mask]).abs().max().item() <= TOL, (c["key"], list(sel))


@pytest.mark.parametrize("scene", SCENES + ["overlap"])
def test_stamps_are_exact_and_a_second_stamp_equals_a_fresh_build(dev, scene):
    """The owner grid and the cell lists as indices; after every person moved, the stamp that clears the listed cells first leaves exactly
    the grid of a fresh build (no full-map clear ever runs)."""
    g = M.scene_group_size(scene)
    rb = torch.from_numpy(Z[f"{scene}/rb"])
    n = rb.shape[0]
    owner = torch.zeros(n // g, *HS.shape, dtype=torch.int32, device=dev)
    cells = torch.full((n, M.ROOT_POINTS), -1, dtype=torch.int32, device=dev)
    ops.crowd_stamp(rb.to(dev), g, owner, cells)
    assert torch.equal(cells.cpu().long(), M.stamp_cells(rb, *HS.shape))
    assert torch.equal(owner.cpu(), M.owner_grid(rb, g, *HS.shape))
    assert torch.equal(owner.cpu() > 0, M.stamped_mask(Z, f"{scene}/stamped", n // g))
    if f"{scene}/rb2" not in Z.files:
        return
    rb2 = torch.from_numpy(Z[f"{scene}/rb2"])
    ops.crowd_stamp(rb2.to(dev), g, owner, cells)                                           # clears the first frame's cells, then stamps
    assert torch.equal(cells.cpu().long(), M.stamp_cells(rb2, *HS.shape))
    assert torch.equal(owner.cpu(), M.owner_grid(rb2, g, *HS.shape))
    assert torch.equal(owner.cpu() > 0, M.stamped_mask(Z, f"{scene}/stamped2", n // g))
    ops.crowd_stamp(rb.to(dev), g, owner, cells, clear=False)                               # without the clear both frames remain
    assert torch.equal(owner.cpu() > 0, (M.owner_grid(rb, g, *HS.shape) > 0) | (M.owner_grid(rb2, g, *HS.shape) > 0))


@pytest.mark.parametrize("kind,root,center", [("group_obs", "head", True), ("stamps", "root", False), ("stamps_velocity", "head", False),
                                              ("velocity", "root", True)])
def test_terrain_env_observation_over_three_steps(dev, kind, root, center):
    """HumanoidPedestrianTerrainZ: the observation after a full reset, after each of 3 steps of SyntheticTaskSim and after a partial reset
    equals the model on the simulator's state.  The stand-in replays the two conditioned frames of the (24, 6) scene in turn."""
    over = dict(configs.crowd_env(kind, num_env_group=6), sensor_res=8, terrain_obs_root=root, use_center_height=center)
    vec_env, _ = configs.make_env(24, 1, str(dev), env_kind="terrain_z", env_overrides=over)
    task = vec_env.env.task
    for f, key in enumerate(("n24g6/rb", "n24g6/rb2")):
        task.sim.bank["rb"][f][:, M.FILLED] = torch.from_numpy(Z[key])[:, M.FILLED].to(dev)
    task.sim.rigid_body_state.copy_(task.sim.bank["rb"][0])
    hp = syn.square_height_points(2.0, 8)
    hw = 64 * (3 if "velocity" in kind else 1)
    width = hw + (165 if kind == "group_obs" else 0)
    assert task.get_task_obs_size() == 20 + width
    col = task.get_self_obs_size() + 20

    def check(rows=slice(None)):
        torch.cuda.synchronize()
        rbc = task.sim.rigid_body_state.cpu()
        want = M.crowd_blocks(rbc, HS, hp, CP, kind, 6, upright=True, sensor_body=M.HEAD if root == "head" else 0, use_center_height=center)
        got = task.obs_buf[:, col:].cpu()
        assert got.shape == want.shape
        assert (got[rows] - want[rows]).abs().max().item() <= TOL
        return got

    task.reset()
    first = check()
    gen = torch.Generator(device=dev).manual_seed(3)
    for step in range(3):
        task.step(torch.randn(24, 32, device=dev, generator=gen))
        got = check()
        assert torch.isfinite(task.obs_buf).all() and torch.isfinite(task.rew_buf).all()
        assert not torch.equal(got, first) or step == 1                                    # the stand-in alternates between its two frames
    ids = torch.tensor([1, 7, 13, 22], device=dev)
    task._obs_store.fill_(float("nan"))
    task.reset(ids)
    got = check(ids.cpu())
    keep = torch.ones(24, dtype=torch.bool)
    keep[ids.cpu()] = False
    assert torch.isnan(got[keep]).all() and (task.progress_buf[ids] == 0).all()


@pytest.mark.parametrize("kind", ["group_obs", "stamps_velocity"])
def test_crowd_config_trains_two_epochs(dev, kind):
    # (the config's own overrides switch group_obs on: another kind has to switch it off again)
    over = configs.crowd_env(kind, num_env_group=16, sensor_res=8, group_obs=False) if kind != "group_obs" else None
    agent, _ = configs.make_agent("terrain_z_crowd_small", device=str(dev), seed=5, env_overrides=over)
    task = agent.vec_env.env.task
    want = {"group_obs": {"traj": 20, "heightmap": 1024, "people": 165}, "stamps_velocity": {"traj": 20, "heightmap_velocity": 192}}[kind]
    assert task.get_task_obs_size_detail() == want and task.get_task_obs_size() == sum(want.values())
    assert task.num_obs == task.get_self_obs_size() + sum(want.values()) and task.num_actions == 32 and task._group_num_people == 16
    agent.init_tensors()
    agent.obs = agent.env_reset()
    first = None
    for _ in range(2):
        info = agent.train_epoch()
        assert torch.isfinite(torch.stack(info["actor_loss"])).all()
        first = first if first is not None else agent.model.flat.clone()
    assert torch.isfinite(task.obs_buf).all() and torch.isfinite(agent.model.flat).all() and not torch.equal(first, agent.model.flat)
    blk = task.obs_buf[:, task.get_self_obs_size() + 20:]
    assert blk.abs().max().item() <= 20.0 and blk.std().item() > 0.1


def test_plain_height_block_is_traj_steps_bit_for_bit(dev):
    """pulse_crowd_heights without owner grid and velocity channels and the height block of pulse_traj_step share terrain_math.h's cell
    lookup and centre height, so on the same inputs they are the same bits.  Five envs on the synthetic field; a 7-point grid (traj_step
    takes four points per thread: 7 is no multiple of 4) and the 32 x 32 one (four passes of the one-point-per-thread loop); centre height
    and upright start on and off; env 3 stands on the field's corner, so points leave it on both axes and are clipped to [0, size - 2];
    a mask leaves rows 1 and 4 as they were.  Every combination goes through ops.traj_step: none is left out."""
    from pulse_amd._lib import TASK_OBS
    n, off, head = 5, 6, M.HEAD
    rb = torch.from_numpy(Z["n24g6/rb"])[:n].clone()
    # the corner: the field is 26 m x 30 m (260 x 300 cells of 0.1 m).  Both grids reach 1.41 m or more from the sensor in every direction
    # whatever its heading, so with the head within 1 m of the root on either axis (25.6 - 1 + 1.41 > 25.9, -0.4 + 1 - 1.41 < 0) some
    # point has x past the last cell pair and some point y < 0
    rb[3, :, 0:2] += torch.tensor([25.6, -0.4]) - rb[3, 0, 0:2]
    assert (rb[3, head, 0:2] - rb[3, 0, 0:2]).abs().max() < 1.0
    rb = rb.to(dev)
    seven = torch.tensor([[2.0, 0.0], [-2.0, 0.0], [0.0, 2.0], [0.0, -2.0], [1.5, 1.5], [-1.5, -1.5], [0.3, -0.1]])
    verts = torch.zeros(n, 2, 3, device=dev)
    verts[:, 1, 0] = 1.0
    prog = torch.zeros(n, dtype=torch.int64, device=dev)
    mask = torch.tensor([1, 0, 1, 1, 0], dtype=torch.bool)
    for hp in (seven.to(dev), syn.square_height_points(2.0, 32).to(dev)):
        nh = hp.shape[0]
        for center in (True, False):
            for upright in (True, False):
                kw = dict(upright=upright, sensor_body=head, center_points=CP.to(dev), use_center_height=center)
                crowd = torch.full((n, off + nh + 5), float("nan"), device=dev)
                ops.crowd_heights(rb, HS.to(dev), hp, obs=crowd, obs_offset=off, env_mask=mask.to(dev), **kw)
                traj = torch.full((n, off + 20 + nh + 5), float("nan"), device=dev)
                ops.traj_step(rb, verts, prog, what=TASK_OBS, dt=1.0 / 30.0, episode_dur=10.0, heightsamples=HS.to(dev), height_points=hp,
                              obs=traj, obs_offset=off, env_mask=mask.to(dev), **kw)
                crowd, traj, tag = crowd.cpu(), traj.cpu(), (nh, center, upright)
                assert torch.isnan(crowd[~mask]).all() and torch.isnan(traj[~mask]).all(), tag          # masked rows: poison untouched
                assert torch.isnan(crowd[:, :off]).all() and torch.isnan(crowd[:, off + nh:]).all(), tag
                got, want = crowd[mask, off:off + nh], traj[mask, off + 20:off + 20 + nh]
                assert torch.isfinite(got).all() and torch.equal(got, want), tag


def test_error_statuses_and_wrapper_checks(dev):
    lib = _lib.load()
    rb = torch.from_numpy(Z["n24g6/rb"]).to(dev)
    obs = torch.zeros(24, 256, device=dev)
    err = lambda: lib.pulse_last_error().decode()

    def group_args(**kw):
        a = _lib.CrowdGroupObsArgs()
        a.num_envs, a.group_size, a.rb, a.rb_env_stride, a.num_bodies, a.upright_start = 24, 6, rb.data_ptr(), rb.stride(0), 24, 1
        a.obs, a.obs_stride, a.obs_offset = obs.data_ptr(), obs.stride(0), 0
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    assert lib.pulse_crowd_group_obs(None, None) == -1 and "null args" in err()
    assert lib.pulse_crowd_group_obs(group_args(group_size=4), None) == -1 and "< 6" in err()
    assert lib.pulse_crowd_group_obs(group_args(group_size=7), None) == -1 and "not a multiple" in err()
    assert lib.pulse_crowd_group_obs(group_args(rb=None), None) == -1 and "rigid-body" in err()
    assert lib.pulse_crowd_group_obs(group_args(obs=None), None) == -1 and "obs" in err()
    assert lib.pulse_crowd_group_obs(group_args(num_bodies=20), None) == -1
    assert lib.pulse_crowd_group_obs(group_args(obs_stride=100), None) == -1
    assert lib.pulse_crowd_group_obs(group_args(num_envs=0), None) == 0                     # no work is no error
    assert lib.pulse_crowd_stamp(None, None) == -1 and lib.pulse_crowd_heights(None, None) == -1
    s = _lib.CrowdStampArgs()
    s.num_envs, s.group_size, s.rb, s.rb_env_stride, s.map_rows, s.map_cols, s.horizontal_scale = 24, 5, rb.data_ptr(), rb.stride(0), 260, 300, 0.1
    assert lib.pulse_crowd_stamp(ctypes.byref(s), None) == -1 and "not a multiple" in err()
    s.group_size = 6
    assert lib.pulse_crowd_stamp(ctypes.byref(s), None) == -1 and "null owner" in err()
    h = _lib.CrowdHeightsArgs()
    h.num_envs, h.rb, h.rb_env_stride, h.num_bodies = 24, rb.data_ptr(), rb.stride(0), 24
    assert lib.pulse_crowd_heights(ctypes.byref(h), None) == -1 and "height field" in err()
    # the wrappers refuse what the kernels would misread
    owner = torch.zeros(4, 260, 300, dtype=torch.int32, device=dev)
    cells = torch.full((24, 200), -1, dtype=torch.int32, device=dev)
    hp = syn.square_height_points(2.0, 8).to(dev)
    with pytest.raises(ValueError, match="topk"):
        ops.crowd_group_obs(rb, 4)
    with pytest.raises(ValueError, match="not a multiple"):
        ops.crowd_group_obs(rb, 7)
    with pytest.raises(TypeError):
        ops.crowd_group_obs(rb.double(), 6)
    with pytest.raises(ValueError):
        ops.crowd_group_obs(rb.cpu(), 6)
    with pytest.raises(TypeError):
        ops.crowd_stamp(rb, 6, owner.long(), cells)
    with pytest.raises(TypeError):
        ops.crowd_stamp(rb, 6, owner, cells.long())
    with pytest.raises(ValueError):
        ops.crowd_stamp(rb, 6, owner[:2], cells)
    with pytest.raises(TypeError):
        ops.crowd_heights(rb, HS.to(dev).int(), hp)
    with pytest.raises(TypeError):
        ops.crowd_heights(rb, HS.to(dev), hp, group_size=6, owner=owner.float())
    with pytest.raises(ValueError):
        ops.crowd_heights(rb, HS.to(dev), hp, group_size=12, owner=owner)
