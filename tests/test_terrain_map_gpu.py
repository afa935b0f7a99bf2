"""GPU: the kernels of csrc/terrain_map.hip (pulse_terrain_walkable, pulse_terrain_valid_cells, pulse_terrain_sample) bit for bit against
tests/terrain_map_model.py -- which tests/test_terrain_map_cpu.py holds to the reference -- and the terrain task resetting onto a Terrain.

Shapes: maps of 37 x 131 and 9 x 300 cells (several 256-column passes, widths that are no multiple of 64 or 256), 1 x 70 (one row: nothing is
kept) and 5 x 600 (rows wider than two workgroup passes); borders 0 and 3; tiles of 8 x 8 cells and of one cell.
"""
import numpy as np
import pytest
import torch

import task_reset_model as M
import terrain_map_model as TM
from oracle.motion_oracle import OracleMotionLib
from pulse_amd import configs, ops, synthetic as syn

pytestmark = pytest.mark.gpu

NAN = float("nan")


def tile_grid(shape, border, tile):
    """Tiles that cover the map inside the border; the last row / column of tiles may be cut off by the array's end."""
    return -(-(shape[0] - 2 * border) // tile), -(-(shape[1] - 2 * border) // tile)


def walkable_scenarios(shape, border, tile):
    """(name, heights, tile_flags or None, mask or None) on a map of ``shape``: tiles of ``tile`` x ``tile`` cells from ``border`` on (cells
    past the last whole tile belong to none)."""
    g = np.random.RandomState(shape[1] + 10 * border + tile)
    tr, tc = tile_grid(shape, border, tile)
    heights = (g.randint(-40, 40, size=shape) * (g.rand(*shape) < 0.15)).astype(np.int16)
    flags = (g.rand(tr, tc) < 0.3).astype(np.uint8)
    out = [("random", heights, flags, None)]
    # a flagged tile in the map's corner with its corner cell and its far edge raised, next to an unflagged tile full of non-zero heights:
    # the dilation crosses into the neighbour, the neighbour's own heights are no obstacles
    h = np.zeros(shape, dtype=np.int16)
    f = np.zeros((tr, tc), dtype=np.uint8)
    f[0, 0] = 1
    h[border, border] = 7
    h[border:border + tile, border + tile - 1] = -3
    h[border:border + tile, border + tile:border + 2 * tile] = 11
    h[shape[0] - 1, shape[1] - 1] = 5                                                      # outside every flagged tile
    out.append(("edge_next_to_unflagged", h, f, None))
    out.append(("all_obstacle", np.full(shape, 9, dtype=np.int16), np.ones((tr, tc), dtype=np.uint8), None))
    out.append(("none", heights, np.zeros((tr, tc), dtype=np.uint8), None))
    mask = g.rand(*shape) < 0.02
    mask[0, 0] = mask[-1, -1] = mask[0, -1] = mask[-1, 0] = True
    out.append(("mask_only", None, None, mask))
    out.append(("mask_and_tiles", heights, flags, mask))
    return out


@pytest.mark.parametrize("shape", [(37, 131), (9, 300)])
def test_walkable_equals_model(dev, shape):
    checked = 0
    for border in (0, 3):
        for tile in (8, 1):
            for name, heights, flags, mask in walkable_scenarios(shape, border, tile):
                obst = TM.obstacles(heights, flags, border, tile, tile, mask)
                if name == "edge_next_to_unflagged":
                    edge = min(tile, shape[0] - border)                                    # the raised edge column, cut off by the array's end
                    assert obst.sum() == edge + (0 if tile == 1 else 1) and not obst[:, border + tile:].any()
                if name == "all_obstacle" and border == 0 and tile == 1:
                    assert obst.all()
                for k in (0, 1, 3):
                    want = TM.walkable(obst, k)
                    kw = {}
                    if flags is not None:
                        kw.update(tile_flags=torch.from_numpy(flags).to(dev), border=border, length_px=tile, width_px=tile)
                    if mask is not None:
                        kw["obstacle_mask"] = torch.from_numpy(mask).to(dev)
                    got = ops.terrain_walkable(None if heights is None else torch.from_numpy(heights).to(dev), iterations=k, **kw)
                    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(want)), (name, border, tile, k)
                    checked += 1
                if name == "edge_next_to_unflagged":
                    assert want[border, min(border + tile + 2, shape[1] - 1)] == 1        # (k = 3) the dilation crossed the tile's edge
    print(f"[terrain map] walkable {shape}: {checked} fields equal the model")


def test_walkable_wrapper_rejects_what_the_kernel_cannot_read(dev):
    h = torch.zeros(9, 12, dtype=torch.int16, device=dev)
    with pytest.raises(TypeError, match="tile_flags .* or obstacle_mask"):
        ops.terrain_walkable(h)
    with pytest.raises(ValueError, match="obstacle_mask"):
        ops.terrain_walkable(h, tile_flags=torch.ones(1, 1, dtype=torch.uint8, device=dev), length_px=8, width_px=8,
                             obstacle_mask=torch.zeros(9, 13, dtype=torch.bool, device=dev))
    with pytest.raises(Exception, match="iterations must be 0 .. 16"):
        ops.terrain_walkable(h, obstacle_mask=torch.zeros(9, 12, dtype=torch.bool, device=dev), iterations=17)


def valid_fields(shape):
    g = np.random.RandomState(shape[0] * 1000 + shape[1])
    w = (g.rand(*shape) < 0.2).astype(np.uint8)
    out = [("random", w)]
    if shape[0] >= 5:
        v = w.copy()
        v[shape[0] // 2] = 1                                                               # a row with no kept cell between rows with some
        v[shape[0] // 2 - 1] = 0                                                           # and a fully kept one
        out.append(("empty_and_full_rows", v))
        v = w.copy()
        v[0] = v[1] = 1                                                                    # the candidates' extent starts at row 2: data-dependent bounds
        v[:, -3:] = 1
        out.append(("shifted_bounds", v))
    out.append(("all_walkable", np.zeros(shape, dtype=np.uint8)))
    out.append(("nothing_walkable", np.ones(shape, dtype=np.uint8)))
    return out


@pytest.mark.parametrize("shape", [(37, 131), (9, 300), (1, 70), (5, 600)])
def test_valid_cells_equal_model(dev, shape):
    from pulse_amd.env.terrain import border_scaled
    cells = shape[0] * shape[1]
    kept = []
    for border in (0, 3):
        for name, w in valid_fields(shape):
            wx, wy = TM.valid_cells(w, border)
            n = wx.numel()
            x, y = (torch.full((cells + 7,), NAN, device=dev) for _ in range(2))
            gx, gy, count = ops.terrain_valid_cells(torch.from_numpy(w).to(dev), border_scaled=border_scaled(border), coord_x=x, coord_y=y)
            assert gx.data_ptr() == x.data_ptr() and count.dtype == torch.int64 and int(count.item()) == n, (name, border)
            assert torch.equal(x[:n].cpu(), wx) and torch.equal(y[:n].cpu(), wy), (name, border)             # table and order
            assert torch.isnan(x[n:]).all() and torch.isnan(y[n:]).all(), (name, border)                   # the tail keeps its fill
            kept.append(n)
            if n > 9:                                                                      # a table that is too short is filled and not overrun
                big = torch.full((2, n + 5), NAN, device=dev)
                _, _, count = ops.terrain_valid_cells(torch.from_numpy(w).to(dev), border_scaled=border_scaled(border), coord_x=big[0, :n - 9],
                                                      coord_y=big[1, :n - 9])
                assert int(count.item()) == n and torch.equal(big[0, :n - 9].cpu(), wx[:n - 9]) and torch.equal(big[1, :n - 9].cpu(), wy[:n - 9])
                assert torch.isnan(big[:, n - 9:]).all()
    print(f"[terrain map] valid cells {shape}: kept {kept}")
    assert (max(kept) > 0) == (shape[0] > 1)                                               # one row: x < xmax fails everywhere, as in the reference


def test_sample_equals_model(dev):
    n, m, p = 64, 1000, 16
    g = torch.Generator().manual_seed(3)
    cx, cy = torch.rand(m, generator=g) * 100, torch.rand(m, generator=g) * 100
    idx = torch.randint(0, m, (n,), generator=g)
    idx[0], idx[1], idx[63] = 0, m - 1, m - 1
    third = torch.zeros(n, dtype=torch.bool)
    third[::3] = True
    below_one = float(np.nextafter(np.float32(1), np.float32(0)))
    u = [torch.rand(n // p, generator=g), torch.rand(n // p, generator=g), torch.rand(n // p, p, generator=g), torch.rand(n // p, p, generator=g)]
    u[0][0], u[1][0], u[2][0, 0], u[3][0, 0] = 0.0, below_one, 0.0, 0.0
    u[0][1], u[1][1], u[2][0, 1], u[3][0, 1], u[2][3, 15], u[3][3, 15] = below_one, 0.0, below_one, below_one, below_one, 0.0
    want_table = TM.sample_table(cx, cy, idx)
    want_groups = TM.sample_groups(16, 32, *u)
    d = lambda t: t.to(dev)
    for name, mask in (("all", torch.ones(n, dtype=torch.bool)), ("none", torch.zeros(n, dtype=torch.bool)), ("every_third", third), ("no_mask", None)):
        rows = torch.ones(n, dtype=torch.bool) if mask is None else mask
        out = torch.full((n, 2), NAN, device=dev)
        ops.terrain_sample(out, coord_x=d(cx), coord_y=d(cy), idx=d(idx), env_mask=None if mask is None else d(mask))
        assert torch.equal(out.cpu()[rows], want_table[rows]) and torch.isnan(out.cpu()[~rows]).all(), name
        out = torch.full((n, 2), NAN, device=dev)
        ops.terrain_sample(out, env_mask=None if mask is None else d(mask), group_num_people=p, extent_x=16, extent_y=32,
                           u_center=d(torch.stack(u[:2])), u_dx=d(u[2]), u_dy=d(u[3]))
        assert torch.equal(out.cpu()[rows], want_groups[rows]) and torch.isnan(out.cpu()[~rows]).all(), name
    assert want_groups[0, 0] == -8.0 and below_one < 1.0                                  # u = 0: the centre at 0, the offset at its lower end
    # an index outside the table writes nothing
    bad = idx.clone()
    bad[5], bad[6] = m, -1
    out = torch.full((n, 2), NAN, device=dev)
    ops.terrain_sample(out, coord_x=d(cx), coord_y=d(cy), idx=d(bad))
    assert torch.isnan(out[5:7]).all() and torch.equal(out.cpu()[7:], want_table[7:])
    with pytest.raises(ValueError, match="idx"):
        ops.terrain_sample(out, coord_x=d(cx), coord_y=d(cy), idx=d(idx[:-1]))
    with pytest.raises(ValueError, match="not a multiple"):
        ops.terrain_sample(out, group_num_people=24, u_center=d(u[0]), u_dx=d(u[2]), u_dy=d(u[3]))


def test_terrain_object_equals_model(dev):
    """Terrain.from_height_field on a small map with a tile grid: fields, table, count; both draws into the right rows."""
    from pulse_amd.env.terrain import Terrain
    g = np.random.RandomState(5)
    border, tile, tr, tc = 4, 8, 3, 5
    shape = (2 * border + tr * tile, 2 * border + tc * tile)
    heights = (g.randint(1, 50, size=shape) * (g.rand(*shape) < 0.03)).astype(np.int16)
    flags = np.array([[1, 0, 0, 1, 0], [0, 0, 1, 0, 0], [0, 1, 0, 0, 0]], dtype=np.uint8)
    t = Terrain.from_height_field(heights, border=border, tile_flags=flags, tile_shape=(tile, tile), device=dev)
    walk = TM.walkable(TM.obstacles(heights, flags, border, tile, tile), 3)
    wx, wy = TM.valid_cells(walk, border)
    assert torch.equal(t.walkable_field.cpu(), torch.from_numpy(walk)) and torch.equal(t.heightsamples.cpu(), torch.from_numpy(heights))
    assert t.num_samples == wx.numel() > 0 and torch.equal(t.coord_x_scale.cpu(), wx) and torch.equal(t.coord_y_scale.cpu(), wy)
    assert (t.sample_extent_x, t.sample_extent_y, t.tot_rows, t.tot_cols) == (int(tr * tile * 0.1), int(tc * tile * 0.1)) + shape
    gen = torch.Generator(device=dev).manual_seed(9)
    out = torch.full((32, 2), NAN, device=dev)
    mask = torch.arange(32, device=dev) % 2 == 0
    t.sample_into(out, mask, gen)
    table = {(a, b) for a, b in zip(wx.tolist(), wy.tolist())}
    assert all((a, b) in table for a, b in out[mask].cpu().tolist()) and torch.isnan(out[~mask]).all()
    locs = t.sample_valid_locations(32, torch.arange(5, device=dev), generator=gen)
    assert locs.shape == (5, 2) and all((a, b) in table for a, b in locs.cpu().tolist())
    grp = t.sample_valid_locations(32, torch.tensor([3, 20], device=dev), 16, True, generator=gen)
    assert grp.shape == (2, 2) and torch.isfinite(grp).all()
    with pytest.raises(ValueError, match="not a multiple"):
        t.sample_valid_locations(30, None, 16, True, generator=gen)
    with pytest.raises(ValueError, match="no valid start cell"):
        Terrain.from_height_field(np.zeros((3, 40), dtype=np.int16), border=1, obstacle_mask=np.ones((3, 40), dtype=bool), device=dev)


# ------------------------------------------------------------------------------------------------------------------ the task
@pytest.fixture(scope="module")
def agent(dev):
    torch.manual_seed(5)
    ag, _ = configs.make_agent("terrain_z_amp_small", device=str(dev), seed=99, terrain="poles_small")
    return ag


def test_env_resets_onto_valid_cells(agent, dev):
    task = agent.vec_env.env.task
    sim, terrain, n = task.sim, task.sim.terrain, task.num_envs
    assert task._terrain is terrain and task._heightsamples.data_ptr() == terrain.heightsamples.data_ptr()
    assert terrain.heightsamples.shape == (1160, 1320) and terrain.tile_kinds == [["poles", "poles", "flat", "flat"]] * 2
    walk = terrain.walkable_field.cpu()
    assert walk.sum() > 0 and (terrain.heightsamples != 0).sum() > 0                       # there are poles
    table = {(a, b) for a, b in zip(terrain.coord_x_scale.tolist(), terrain.coord_y_scale.tolist())}
    assert len(table) == terrain.num_samples
    lib = OracleMotionLib(syn.synthetic_motion_library(syn.make_generator(99 + 5, 0), n))
    state = lambda: (sim.rigid_body_state.cpu().clone(), sim.dof_pos.cpu().clone(), sim.dof_vel.cpu().clone())
    for mask in (torch.ones(n, dtype=torch.bool), torch.arange(n) % 3 == 0):
        before = state()
        task.reset_masked(mask.to(dev))
        rb, dp, dv = state()
        xy = rb[mask, 0, 0:2]
        assert torch.equal(xy, task._new_root_xy.cpu()[mask])
        assert all((a, b) in table for a, b in xy.tolist())                                # exact membership in the valid table
        cell = (xy / 0.1).round().long()
        assert (walk[cell[:, 0], cell[:, 1]] == 0).all()                                   # nobody stands on the dilated obstacle field
        assert torch.equal(rb[~mask], before[0][~mask]) and torch.equal(dp[~mask], before[1][~mask]) and torch.equal(dv[~mask], before[2][~mask])
        # root height: the motion's plus the mean centre height at the new place (tests/task_reset_model.py).  Every root sits exactly on a
        # cell corner here, so a centre sample may take either neighbouring cell (tests/test_task_reset_gpu.py): where the map is flat for
        # five cells around that cannot matter and the height is the model's to 1e-5; elsewhere the lift is a mean of heights of that
        # neighbourhood and lies between its lowest and highest.  test_root_is_lifted_onto_a_plateau holds a non-zero lift to the model.
        ids, times = task._reset_ref_motion_ids.cpu(), task._reset_ref_motion_times.cpu()
        centre = torch.cat([task._center_points.cpu(), torch.zeros(9, 1)], dim=1)
        hs = task._heightsamples.cpu()
        m = M.ref_state(lib, ids, times, "terrain", new_root_xy=task._new_root_xy.cpu(), heightsamples=hs, center_points=centre)
        ground = M.ref_state(lib, ids, times, "terrain", new_root_xy=task._new_root_xy.cpu(), heightsamples=torch.zeros_like(hs), center_points=centre)
        err = (rb[:, 0, 2] - m["records"][:, 0, 2]).abs()[mask]
        lift = (rb[:, 0, 2] - ground["records"][:, 0, 2])[mask]
        around = [hs[r - 5:r + 6, c - 5:c + 6].float() * 0.005 for r, c in cell.tolist()]
        flat = torch.tensor([bool((a == 0).all()) for a in around])
        lo, hi = torch.stack([a.min() for a in around]), torch.stack([a.max() for a in around])
        print(f"[terrain map] reset of {int(mask.sum())} envs: largest root-height error {err.max().item():.2e}, {int(flat.sum())} on flat ground")
        assert flat.any() and (err[flat] <= 1e-5).all()
        assert ((lift >= lo - 1e-5) & (lift <= hi + 1e-5)).all()


def test_root_is_lifted_onto_a_plateau(dev):
    """A non-zero lift that no cell edge can change: columns below 26 of the map stand 1 m high, the others 0.3 m; the step runs through
    the middle of a column of flagged tiles (all of it an obstacle), seven cells from the nearest valid cell, and the nine centre samples
    of a root reach less than four cells.  The root height is the motion's plus exactly its plateau's, to 1e-5, for every reset env."""
    from pulse_amd.env.terrain import Terrain
    n, border, tile = 64, 6, 8
    heights = np.full((2 * border + 3 * tile, 2 * border + 5 * tile), 200, dtype=np.int16)
    step = border + 2 * tile + tile // 2
    heights[:, step:] = 60
    flags = np.zeros((3, 5), dtype=np.uint8)
    flags[:, 2] = 1
    terrain = Terrain.from_height_field(heights, border=border, tile_flags=flags, tile_shape=(tile, tile), device=dev)
    cols = (terrain.coord_y_scale / 0.1).round().long().cpu()
    assert ((cols <= step - 7) | (cols >= step + 7)).all() and (cols < step).any() and (cols > step).any()
    env, _ = configs.make_env(n, 16, dev, seed=31, env_kind="terrain_z", env_overrides={"enable_amp_obs": True, "numAMPObsSteps": 2, "amp_seed": 5},
                              terrain=terrain)
    task = env.task
    assert task._terrain is terrain
    lib = OracleMotionLib(syn.synthetic_motion_library(syn.make_generator(31 + 5, 0), n))
    centre = torch.cat([task._center_points.cpu(), torch.zeros(9, 1)], dim=1)
    for mask in (torch.ones(n, dtype=torch.bool), torch.arange(n) % 3 == 1):
        task.reset_masked(mask.to(dev))
        z, xy = task.sim.rigid_body_state[:, 0, 2].cpu(), task._new_root_xy.cpu()
        ids, times = task._reset_ref_motion_ids.cpu(), task._reset_ref_motion_times.cpu()
        hs = task._heightsamples.cpu()
        m = M.ref_state(lib, ids, times, "terrain", new_root_xy=xy, heightsamples=hs, center_points=centre)
        ground = M.ref_state(lib, ids, times, "terrain", new_root_xy=xy, heightsamples=torch.zeros_like(hs), center_points=centre)
        err = (z - m["records"][:, 0, 2]).abs()[mask]
        lift = (z - ground["records"][:, 0, 2])[mask]
        plateau = torch.where((xy[mask, 1] / 0.1).round() < step, 200 * 0.005, 60 * 0.005).float()
        print(f"[terrain map] plateau reset of {int(mask.sum())} envs: largest root-height error {err.max().item():.2e}, "
              f"largest lift error {(lift - plateau).abs().max().item():.2e}, {int((plateau > 0.5).sum())} on the high side")
        assert (err <= 1e-5).all() and ((lift - plateau).abs() <= 1e-5).all()
        assert (plateau > 0.5).any() and (plateau < 0.5).any()


def test_agent_trains_on_the_terrain(agent, dev):
    task = agent.vec_env.env.task
    terrain = task.sim.terrain
    assert task._terrain is terrain
    infos = []
    for e in range(2):
        agent.epoch_num = e + 1
        infos.append(agent.train_epoch())
    torch.cuda.synchronize()
    for info in infos:
        for k in [k for k in info if k.startswith("disc_")] + ["actor_loss", "critic_loss", "grad_norm"]:
            v = info[k]
            v = v if isinstance(v, torch.Tensor) else torch.stack([torch.as_tensor(x, device=dev).float() for x in v])
            assert torch.isfinite(v).all(), k
    assert torch.isfinite(agent.model.flat).all()
    # whatever the rollouts reset went onto valid cells (a row no reset has written yet is still zero)
    xy = task._new_root_xy.cpu()
    xy = xy[(xy != 0).any(dim=1)]
    table = {(a, b) for a, b in zip(terrain.coord_x_scale.tolist(), terrain.coord_y_scale.tolist())}
    assert xy.shape[0] > 0 and all((a, b) in table for a, b in xy.tolist())


def test_without_a_terrain_the_draw_is_the_uniform_one(dev):
    """The one test of this file that passes without the feature too: that is its point (hence the imports inside the other tests)."""
    n = 9
    env, _ = configs.make_env(n, 16, dev, seed=31, env_kind="terrain_z", env_overrides={"enable_amp_obs": True, "numAMPObsSteps": 2, "amp_seed": 5})
    task = env.task
    assert getattr(task, "_terrain", None) is None and not hasattr(task.sim, "terrain")
    twin = torch.Generator(device=dev)
    twin.set_state(task._amp_gen.get_state())
    env.reset(None)
    ids = task._motion_lib.sample_motions(n, generator=twin)                                # the draws of _reset_ref_state_init, in its order
    task._motion_lib.sample_time_interval(ids, generator=twin)
    rows, cols = task._heightsamples.shape
    extent = torch.tensor([rows * 0.1, cols * 0.1], device=dev)
    want = 3.0 + torch.rand(n, 2, device=dev, generator=twin) * (extent - 2 * 3.0)
    assert torch.equal(task._reset_ref_motion_ids, ids) and torch.equal(task._new_root_xy, want)
    assert torch.equal(task._amp_gen.get_state(), twin.get_state())                        # the same generator consumption
