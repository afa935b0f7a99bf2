"""Record tests/golden/crowd.npz: the crowd variant of HumanoidPedestrianTerrain computed by the REFERENCE's own text.

    python tools/gen_golden_crowd.py            (needs the reference tree, oracle/refload.py: PULSE_REFERENCE_ROOT)

Executed as reference text on stubs (oracle.refload: AST-extracted, decorators dropped, nothing copied into this repository):
  compute_group_observation                                   humanoid_pedestrian_terrain.py:1700-1753
  HumanoidPedestrianTerrain.get_heights / _compute_task_obs   :718-772, 385-439
  HumanoidPedestrianTerrain.init_root_points                  :643-660
  Terrain.world_points_to_map / sample_height_points          :1191-1276
The reference never assigns ``self.selected_group_jts`` (compute_group_observation overwrites the argument), so the stub supplies None.
The trajectory samples are zeros: the golden keeps the columns BEHIND the trajectory block, [height block | people block].

The file holds inputs and outputs only.  Scenes come from tests/crowd_model.py (make_scene: rejection sampling of the fixture
conditions); for the larger scenes the outputs are kept for the env subset ``rows`` -- computed by the reference with ``env_ids = rows``,
which is how it serves a partial reset -- so the file stays small.  The stamped cells of every group are kept as a packed bit mask.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import crowd_model as M                                     # noqa: E402
from oracle import refload                                  # noqa: E402
from pulse_amd import synthetic as syn                      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "crowd.npz")
NUM_TRAJ = 10


def _reference():
    T = refload.terrain_functions()
    ns = T["HumanoidPedestrianTerrain.get_heights"].__globals__          # the namespace the terrain file's text runs in
    tf = os.path.join(refload.REFERENCE_ROOT, "phc", "env", "tasks", "humanoid_pedestrian_terrain.py")
    if "compute_group_observation" not in ns:
        for name, text in refload._extract(tf, ["compute_group_observation"]).items():
            exec(compile(text, f"<reference:{name}>", "exec"), ns)
        for name, text in refload._extract(tf, ["init_root_points"], methods_of="HumanoidPedestrianTerrain").items():
            exec(compile(text, f"<reference:HumanoidPedestrianTerrain.{name}>", "exec"), ns)
    return T, ns


def _stub(T, ns, rb, hs, res, kind, group_size, upright, sensor, center):
    n = rb.shape[0]
    hp, cp = M.TO_pad3(syn.square_height_points(2.0, res)), M.TO_pad3(syn.center_height_points())
    terrain = refload.stub_self(heightsamples=hs, horizontal_scale=M.HSCALE, vertical_scale=M.VSCALE)
    terrain.world_points_to_map = lambda pts: T["Terrain.world_points_to_map"](terrain, pts)
    terrain.sample_height_points = lambda pts, **kw: T["Terrain.sample_height_points"](terrain, pts, **kw)
    divide = kind != "velocity"
    env = refload.stub_self(
        cfg={"env": {"terrain": {"terrainType": "trimesh"}, "use_center_height": center}}, num_envs=n, device="cpu", humanoid_type="smpl",
        _has_upright_start=upright, num_height_points=hp.shape[0], num_center_height_points=cp.shape[0],
        height_points=hp[None].repeat(n, 1, 1), center_height_points=cp[None].repeat(n, 1, 1),
        velocity_map=kind in ("stamps_velocity", "velocity"), _divide_group=divide, _group_obs=kind == "group_obs", _disable_group_obs=False,
        terrain=terrain, terrain_obs=True, terrain_obs_root=sensor, height_meas_scale=M.MEAS_SCALE, _num_traj_samples=NUM_TRAJ,
        _humanoid_root_states=rb[:, 0].clone(), _rigid_body_pos=rb[..., 0:3].clone(), _rigid_body_rot=rb[..., 3:7].clone(),
        _rigid_body_vel=rb[..., 7:10].clone(), selected_group_jts=None)
    if divide:                                                                            # load_common_humanoid_configs, humanoid.py:256-261
        env._group_num_people = min(group_size, n)
        env._group_ids = torch.tensor(np.arange(n / env._group_num_people).repeat(env._group_num_people).astype(int))
    env.root_points = ns["init_root_points"](env)
    env.get_heights = lambda root_states, env_ids=None: T["HumanoidPedestrianTerrain.get_heights"](env, root_states=root_states, env_ids=env_ids)
    env.get_center_heights = lambda root_states, env_ids=None: T["HumanoidPedestrianTerrain.get_center_heights"](env, root_states=root_states, env_ids=env_ids)
    env.get_head_pose = lambda env_ids=None: (rb[:, M.HEAD, 0:7] if env_ids is None else rb[env_ids, M.HEAD, 0:7]).clone()
    env._fetch_traj_samples = lambda env_ids=None: torch.zeros(n if env_ids is None else len(env_ids), NUM_TRAJ, 3)
    return env


def reference_blocks(rb, hs, res, kind, group_size, upright, sensor, center, env_ids=None):
    """_compute_task_obs of the reference on a stub, minus the trajectory block: (rows, width)."""
    T, ns = _reference()
    env = _stub(T, ns, rb, hs, res, kind, group_size, upright, sensor, center)
    obs = T["HumanoidPedestrianTerrain._compute_task_obs"](env, env_ids)
    return obs[:, 2 * NUM_TRAJ:].clone()


def reference_stamped(rb, hs, group_size):
    """(num_groups, rows, cols) bool: the cells Terrain.sample_height_points raises, from the expression of get_heights :750-753 evaluated
    with the reference's functions (init_root_points, calc_heading_quat, quat_apply, world_points_to_map)."""
    T, ns = _reference()
    n = rb.shape[0]
    env = refload.stub_self(num_envs=n, device="cpu")
    pts = ns["init_root_points"](env)
    heading = ns["torch_utils"].calc_heading_quat(rb[:, 0, 3:7])
    world = ns["quat_apply"](heading.repeat(1, env.num_root_points).reshape(-1, 4), pts) + rb[:, 0, :3].unsqueeze(1)
    terrain = refload.stub_self(heightsamples=hs, horizontal_scale=M.HSCALE, vertical_scale=M.VSCALE)
    px, py = T["Terrain.world_points_to_map"](terrain, world)
    mask = torch.zeros(n // group_size, hs.shape[0], hs.shape[1], dtype=torch.bool)
    grp = (torch.arange(n) // group_size).repeat_interleave(env.num_root_points)
    mask[grp, px.view(-1), py.view(-1)] = True
    return mask


def generate():
    """dict key -> numpy array.  Runs single-threaded: where footprints share a cell the reference's indexed assignment of the velocities
    (:1241) is well defined only when it runs serially (the last write, the highest env index, wins); split over several CPU threads the
    winner is arbitrary -- neither the first nor the last -- and differs from run to run."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _generate()
    finally:
        torch.set_num_threads(threads)


def _generate():
    hs = syn.synthetic_height_field()
    out = {}

    def record(prefix, rb, res, kinds, combos, group_size, rows):
        ids = None if rows is None else rows
        for kind in kinds:
            for up, sensor, center in (combos if kind != "group_obs" else combos[:2]):
                out[f"{prefix}/{kind}/{M.combo_name(up, sensor, center)}"] = reference_blocks(rb, hs, res, kind, group_size, up, sensor, center, ids).numpy()

    for n, g in M.SHAPES:
        s = M.scene_name(n, g)
        rb = M.make_scene(n, g, disjoint=M.DISJOINT[(n, g)])
        rb2 = M.make_scene(n, g, frame=1, disjoint=M.DISJOINT[(n, g)])
        rows = M.rows_subset(n, g)
        out[f"{s}/rb"], out[f"{s}/rb2"], out[f"{s}/rows"] = rb.numpy(), rb2.numpy(), rows.numpy()
        record(s, rb, 8, M.KINDS, M.COMBOS, g, None if len(rows) == n else rows)
        out[f"{s}/stamped"] = np.packbits(reference_stamped(rb, hs, g).numpy())
        out[f"{s}/stamped2"] = np.packbits(reference_stamped(rb2, hs, g).numpy())
    rb = M.overlap_scene()
    out["overlap/rb"] = rb.numpy()
    record("overlap", rb, 8, ("stamps", "stamps_velocity"), M.COMBOS[:2], 6, None)
    out["overlap/stamped"] = np.packbits(reference_stamped(rb, hs, 6).numpy())
    rb = M.make_scene(24, 6, grids=(8, 32), seed=1)
    rows = torch.tensor([0, 7, 13, 23])
    out["res32/rb"], out["res32/rows"] = rb.numpy(), rows.numpy()
    record("res32", rb, 32, ("stamps_velocity",), M.COMBOS[:1], 6, rows)
    return out


if __name__ == "__main__":
    if not refload.available():
        sys.exit(f"the reference tree is not at {refload.REFERENCE_ROOT}")
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {len(arrays)} arrays, {os.path.getsize(OUT)} bytes")
