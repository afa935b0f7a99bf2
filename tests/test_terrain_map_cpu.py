"""CPU: the walkable map of the terrain task (pulse_amd/env/terrain.py, csrc/terrain_map.hip).

  * tests/terrain_map_model.py (what the GPU tests hold the kernels to) against the reference's own method bodies -- Terrain.__init__,
    curiculum, randomized_terrain and sample_valid_locations (phc/env/tasks/humanoid_pedestrian_terrain.py:1114-1189, 1307-1471), extracted
    and executed with recording stand-ins for the isaacgym.terrain_utils generators -- bit for bit: geometry, every generator's arguments,
    env origins, the height field, the dilated walkable field, the valid-cell table with its order, both sampling modes on seeded draws.
    Live where the reference checkout is present, replayed from tests/golden/ref/test_terrain_map_cpu/ otherwise;
  * the package's host-side layout (terrain.build_layout) against the model on the same cases;
  * the L1-diamond form of the dilation against scipy's;
  * the errors Terrain raises by name before any device is touched; the three entry points' binding and argument errors.
"""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

import terrain_map_model as TM
from oracle import refload
from oracle.refrecord import RefRecord
from pulse_amd import _lib
from pulse_amd.env import terrain as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the terrain block of env_pulse_terrain.yaml (:75-90) at the small_terrain tile size (humanoid_pedestrian_terrain.py:817-819)
SHIPPED = {"terrainType": "trimesh", "staticFriction": 1.0, "dynamicFriction": 1.0, "restitution": 0., "curriculum": True, "mapLength": 8,
           "mapWidth": 8, "numLevels": 5, "numTerrains": 20, "terrainProportions": [0.2, 0.1, 0.15, 0.15, 0.05, 0., 0.25, 0.1],
           "slopeTreshold": 0.9}
RANDOMIZED = dict(SHIPPED, curriculum=False, numLevels=3, numTerrains=5, terrainProportions=[0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.3, 0.1])
# curriculum choices j / 20: smooth slope down (0) and up, rough slope down (0.1) and up, stairs down and up, discrete, stepping, poles, flat
EVERY_BRANCH = dict(SHIPPED, numLevels=2, numTerrains=20, terrainProportions=[0.1, 0.15, 0.1, 0.1, 0.1, 0.1, 0.2, 0.15])
CASES = {"shipped_small_terrain": (SHIPPED, None), "randomized_seeded": (RANDOMIZED, 7), "every_branch": (EVERY_BRANCH, None)}
GEOMETRY = {"border": "border", "width_px": "width_per_env_pixels", "length_px": "length_per_env_pixels", "tot_rows": "tot_rows",
            "tot_cols": "tot_cols", "sample_extent_x": "sample_extent_x", "sample_extent_y": "sample_extent_y"}
REF_GENERATORS = {"pyramid_sloped": "pyramid_sloped_terrain", "random_uniform": "random_uniform_terrain", "pyramid_stairs": "pyramid_stairs_terrain",
                  "discrete_obstacles": "discrete_obstacles_terrain", "stepping_stones": "stepping_stones_terrain", "poles": "poles_terrain"}


def reference_terrain_class(log):
    """The reference's Terrain from its four method bodies, in a namespace that supplies what the module imports around them."""
    path = os.path.join(refload.REFERENCE_ROOT, "phc", "env", "tasks", "humanoid_pedestrian_terrain.py")
    names = ["__init__", "curiculum", "randomized_terrain", "sample_valid_locations"]
    src = refload._extract(path, names, methods_of="Terrain")
    refload._ensure_paths()
    ns = {"np": np, "torch": torch, "ndimage": ndimage, "tqdm": lambda it: it, "SubTerrain": TM.Sub,
          "torch_rand_float": importlib.import_module("isaacgym.torch_utils").torch_rand_float,
          "convert_heightfield_to_trimesh": lambda *a, **k: (None, None)}
    gens = TM.recording_generators(log)
    ns.update({REF_GENERATORS[k]: g for k, g in gens.items()})
    for name in names:
        exec(compile(src[name], f"<reference:Terrain.{name}>", "exec"), ns)
    return type("Terrain", (), {name: ns[name] for name in names})


def group_uniforms(seed, groups, people):
    """The four torch_rand_float draws of sample_valid_locations' group mode (:1178-1179), in its order."""
    torch.manual_seed(seed)
    return (torch.rand(groups, 1).squeeze(1), torch.rand(groups, 1).squeeze(1), torch.rand(groups, people), torch.rand(groups, people))


@pytest.mark.parametrize("case", list(CASES))
def test_model_and_layout_against_reference_bodies(request, case):
    cfg, seed = CASES[case]
    num_robots, ids = 64, torch.tensor([0, 5, 17, 63, 31])
    with RefRecord(request) as R:
        ref, rlog = None, []
        if R.live:
            if seed is not None:
                np.random.seed(seed)
            ref = reference_terrain_class(rlog)(cfg, num_robots, "cpu")
        mlog = []
        if seed is not None:
            np.random.seed(seed)
        m = TM.layout(cfg, TM.recording_generators(mlog), rng=np.random)
        obst = TM.obstacles(m["heights"], m["tile_flags"], m["border"], m["length_px"], m["width_px"])
        walk = TM.walkable(obst, 3)
        cx, cy = TM.valid_cells(walk, m["border"])
        assert obst.any() and m["tile_flags"].any() and not m["tile_flags"].all()            # the case has poles tiles and others

        assert R.obj("geometry", lambda: {k: int(getattr(ref, a)) for k, a in GEOMETRY.items()}) == {k: m[k] for k in GEOMETRY}
        assert R.obj("generator_log", lambda: rlog) == mlog
        assert torch.equal(R.t("env_origins", lambda: torch.from_numpy(ref.env_origins)), torch.from_numpy(m["env_origins"]))
        assert R.matches("height_field_raw", lambda: torch.from_numpy(ref.height_field_raw), torch.from_numpy(m["heights"]))
        assert R.matches("heightsamples", lambda: ref.heightsamples, torch.from_numpy(m["heights"]))
        assert R.matches("walkable_field", lambda: ref.walkable_field.to(torch.uint8), torch.from_numpy(walk))
        if R.live:
            assert set(ref.walkable_field.unique().tolist()) == {0, 1} and ref.coord_x_scale.dtype == torch.float32
        assert R.obj("num_samples", lambda: int(ref.num_samples)) == cx.numel() > 0
        assert R.matches("coord_x_scale", lambda: ref.coord_x_scale, cx) and R.matches("coord_y_scale", lambda: ref.coord_y_scale, cy)

        # sample_valid_locations on seeded draws: the table mode draws from numpy's global stream, the group mode from torch's
        def ref_table():
            np.random.seed(11)
            return ref.sample_valid_locations(num_robots, ids)
        want = R.t("sample_table", ref_table)
        np.random.seed(11)
        idx = np.random.randint(0, cx.numel(), size=ids.shape[0])
        assert torch.equal(TM.sample_table(cx, cy, idx), want)
        for key, env_ids in (("sample_groups_all", None), ("sample_groups_ids", ids)):
            def ref_groups():
                torch.manual_seed(13)
                return ref.sample_valid_locations(num_robots, env_ids, 16, True)
            want = R.t(key, ref_groups)
            got = TM.sample_groups(m["sample_extent_x"], m["sample_extent_y"], *group_uniforms(13, num_robots // 16, 16))
            assert torch.equal(got if env_ids is None else got[env_ids], want) and want.dtype == torch.float32

    # the package's host layout on the same case
    plog = []
    if seed is not None:
        np.random.seed(seed)
    L = PT.build_layout(cfg, num_robots, TM.recording_generators(plog), rng=None)
    assert plog == mlog and L.tile_kinds == m["kinds"]
    assert {k: getattr(L, a) for k, a in GEOMETRY.items()} == {k: m[k] for k in GEOMETRY}
    assert np.array_equal(L.height_field_raw, m["heights"]) and L.height_field_raw.dtype == np.int16
    assert np.array_equal(L.tile_flags, m["tile_flags"]) and np.array_equal(L.env_origins, m["env_origins"])
    if case == "every_branch":
        assert {k for row in m["kinds"] for k in row} == {"smooth_slope-", "smooth_slope", "rough_slope-", "rough_slope", "stairs-", "stairs",
                                                          "discrete", "stepping", "poles", "flat"}


def test_randomized_layout_takes_its_draws_from_rng():
    a = PT.build_layout(RANDOMIZED, 8, TM.recording_generators([]), rng=np.random.RandomState(3))
    np.random.seed(3)
    b = PT.build_layout(RANDOMIZED, 8, TM.recording_generators([]))
    assert a.tile_kinds == b.tile_kinds and np.array_equal(a.height_field_raw, b.height_field_raw)
    c = PT.build_layout(RANDOMIZED, 8, TM.recording_generators([]), rng=np.random.RandomState(4))
    assert a.tile_kinds != c.tile_kinds


@pytest.mark.parametrize("shape", [(1, 70), (9, 9), (37, 131), (64, 300)])
@pytest.mark.parametrize("k", [0, 1, 3])
def test_l1_diamond_is_scipys_dilation(shape, k):
    g = np.random.RandomState(shape[1] + k)
    obst = g.rand(*shape) < 0.01
    obst[0, 0] = obst[-1, -1] = obst[0, -1] = obst[-1, 0] = True
    assert np.array_equal(TM.walkable_l1(obst, k), TM.walkable(obst, k))
    assert np.array_equal(TM.walkable(obst, 0), obst.astype(np.uint8))


def test_valid_cells_model_on_a_small_map():
    """Data-dependent bounds: with a blocked first row the kept band moves down by one row."""
    w = np.zeros((12, 14), dtype=np.uint8)
    x, y = TM.valid_cells(w, 3)
    xs = [float(np.float32(r) * np.float32(0.1)) for r in range(12)]
    b = float(np.float32(3 * 0.1))
    rows = [r for r in range(12) if xs[r] > xs[0] + b and xs[r] < np.float32(xs[11]) - np.float32(b)]
    assert sorted(set((x / 0.1).round().int().tolist())) == rows and x.dtype == torch.float32
    assert torch.equal(x, x.sort().values)                                                    # row-major: x never decreases
    w[0, :] = 1
    x2, _ = TM.valid_cells(w, 3)
    assert x2.min() > x.min()


# ------------------------------------------------------------------------------------------------------------------ errors, no device
def test_from_config_errors_need_no_device():
    gens = TM.recording_generators([])
    with pytest.raises(ValueError, match=r"mapLength 8 != mapWidth 6.*:1320, 1390"):
        PT.Terrain.from_config(dict(SHIPPED, mapWidth=6), 4, gens, "cuda:0")
    for key, fn in (("pyramid_sloped", "pyramid_sloped_terrain"), ("poles", "poles_terrain"), ("pyramid_stairs", "pyramid_stairs_terrain")):
        some = {k: g for k, g in gens.items() if k != key}
        with pytest.raises(NotImplementedError, match=rf"generators\['{key}'\].*isaacgym\.terrain_utils\.{fn}.*humanoid_pedestrian_terrain\.py:1"):
            PT.Terrain.from_config(SHIPPED, 4, some, "cuda:0")
    with pytest.raises(NotImplementedError, match="random_uniform_terrain"):
        PT.Terrain.from_config(SHIPPED, 4, {"pyramid_sloped": gens["pyramid_sloped"]}, "cuda:0")
    with pytest.raises(ValueError, match="terrainType 'plane'"):
        PT.Terrain.from_config(dict(SHIPPED, terrainType="plane"), 4, gens, "cuda:0")
    with pytest.raises(ValueError, match="at least 7 entries"):
        PT.Terrain.from_config(dict(SHIPPED, terrainProportions=[0.5, 0.5]), 4, gens, "cuda:0")
    flat = PT.build_layout(dict(SHIPPED, terrainProportions=[0, 0, 0, 0, 0, 0, 0, 1.]), 4, None)     # the flat kind needs no generator
    assert not flat.height_field_raw.any() and not flat.tile_flags.any()


def test_from_height_field_errors_need_no_device():
    h = np.zeros((22, 30), dtype=np.int16)
    make = lambda *a, **k: PT.Terrain.from_height_field(*a, device="cuda:0", **k)
    with pytest.raises(TypeError, match="int16"):
        make(h.astype(np.int32), border=3, obstacle_mask=h)
    with pytest.raises(ValueError, match="tile_flags .* or obstacle_mask is required"):
        make(h, border=3)
    with pytest.raises(ValueError, match="obstacle_mask .* is not the height field's shape"):
        make(h, border=3, obstacle_mask=np.zeros((22, 31)))
    with pytest.raises(ValueError, match="tile_shape"):
        make(h, border=3, tile_flags=np.ones((2, 3)))
    with pytest.raises(ValueError, match="make a 22 x 33 map"):
        make(h, border=3, tile_flags=np.ones((2, 3)), tile_shape=(8, 9))
    with pytest.raises(ValueError, match="border"):
        make(h, border=-1, obstacle_mask=h)
    flags, shape = PT.check_height_field(h, 3, np.array([[1, 0, 2], [0, 0, 1]]), (8, 8), None)
    assert flags.tolist() == [[1, 0, 1], [0, 0, 1]] and shape == (8, 8) and flags.dtype == np.uint8
    assert PT.border_scaled(3) == float(np.float32(0.30000000000000004)) and PT.border_scaled(500) == 50.0


def test_task_refuses_a_terrain_it_would_ignore():
    """The checks sit before anything goes to the device: a stub simulator is enough."""
    import types
    from pulse_amd import configs
    from pulse_amd.env import humanoid_tasks as HT
    terrain = types.SimpleNamespace(heightsamples=torch.zeros(5, 5, dtype=torch.int16))

    def make(cls, env, **sim):
        cfg = {"env": dict(configs.ENV_TERRAIN_Z, **env), "robot": configs.robot_config("smpl")}
        return cls(cfg, types.SimpleNamespace(num_envs=4, terrain=terrain, **sim), device="cuda:0")
    with pytest.raises(ValueError, match=r"terrain of \(5, 5\) cells and heightsamples of \(4, 5\)"):
        make(HT.HumanoidPedestrianTerrainZ, {}, heightsamples=torch.zeros(4, 5, dtype=torch.int16))
    with pytest.raises(ValueError, match="terrainType is 'plane'"):
        make(HT.HumanoidPedestrianTerrainZ, {"terrain": {"terrainType": "plane"}})
    with pytest.raises(ValueError, match="terrain_obs is off"):
        make(HT.HumanoidPedestrianTerrain, {"terrain_obs": False})


# ------------------------------------------------------------------------------------------------------------------ the entry points
def header_struct_fields(name):
    text = open(os.path.join(ROOT, "include", "pulse_hip.h")).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"[\s\*]", "", part).split(" ")[-1] for part in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    return fields


def test_entry_point_binding():
    lib = _lib.load()
    assert lib.pulse_abi_version() == 36                            # added entry points: no existing struct or signature changed
    for cls, c_name in ((_lib.TerrainWalkableArgs, "terrain_walkable"), (_lib.TerrainValidArgs, "terrain_valid"), (_lib.TerrainSampleArgs, "terrain_sample")):
        assert ctypes.sizeof(cls) == getattr(lib, f"pulse_sizeof_{c_name}_args")()
        assert [f[0] for f in cls._fields_] == header_struct_fields(f"pulse_{c_name}_args"), c_name
    header = open(os.path.join(ROOT, "include", "pulse_hip.h")).read()
    for cite in (":1362-1364, 1380", ":1160-1172", ":1175-1189"):
        assert cite in header
    assert _lib.TERRAIN_MAX_DILATION == int(re.search(r"#define PULSE_TERRAIN_MAX_DILATION (\d+)", header).group(1))
    err = lambda: lib.pulse_last_error()
    fake = ctypes.c_void_p(64)                                      # never dereferenced: every call below returns before a launch

    assert lib.pulse_terrain_walkable(None, None) == -1 and b"null args" in err()
    a = _lib.TerrainWalkableArgs()
    assert lib.pulse_terrain_walkable(ctypes.byref(a), None) == 0   # zero rows: nothing to do
    a.rows, a.cols = -1, 4
    assert lib.pulse_terrain_walkable(ctypes.byref(a), None) == -1 and b"negative map size" in err()
    a.rows, a.walkable, a.obstacle_mask = 4, fake, fake
    for bad in (-1, _lib.TERRAIN_MAX_DILATION + 1):
        a.iterations = bad
        assert lib.pulse_terrain_walkable(ctypes.byref(a), None) == -1 and b"iterations must be 0 .. 16" in err()
    a.iterations, a.obstacle_mask = 3, None
    assert lib.pulse_terrain_walkable(ctypes.byref(a), None) == -1 and b"neither tile_flags nor obstacle_mask" in err()
    a.tile_flags = fake
    assert lib.pulse_terrain_walkable(ctypes.byref(a), None) == -1 and b"tile_flags need heights" in err()
    a.heights = fake
    assert lib.pulse_terrain_walkable(ctypes.byref(a), None) == -1 and b"bad tile grid" in err()
    a.walkable, a.tile_rows, a.tile_cols, a.length_px, a.width_px = None, 1, 1, 4, 4
    assert lib.pulse_terrain_walkable(ctypes.byref(a), None) == -1 and b"null walkable" in err()

    assert lib.pulse_terrain_valid_cells(None, None) == -1 and b"null args" in err()
    v = _lib.TerrainValidArgs()
    assert lib.pulse_terrain_valid_cells(ctypes.byref(v), None) == 0
    v.rows, v.cols = 4, -4
    assert lib.pulse_terrain_valid_cells(ctypes.byref(v), None) == -1 and b"negative map size" in err()
    v.cols = 4
    assert lib.pulse_terrain_valid_cells(ctypes.byref(v), None) == -1 and b"null pointer" in err()
    v.walkable = v.row_extents = v.row_offsets = v.count = fake
    v.capacity = 5
    assert lib.pulse_terrain_valid_cells(ctypes.byref(v), None) == -1 and b"bad output table" in err()
    v.coord_x = v.coord_y = fake
    assert lib.pulse_terrain_valid_cells(ctypes.byref(v), None) == -1 and b"bad scales" in err()

    assert lib.pulse_terrain_sample(None, None) == -1 and b"null args" in err()
    s = _lib.TerrainSampleArgs()
    assert lib.pulse_terrain_sample(ctypes.byref(s), None) == 0     # zero envs
    s.num_envs = -2
    assert lib.pulse_terrain_sample(ctypes.byref(s), None) == -1 and b"negative num_envs" in err()
    s.num_envs = 64
    assert lib.pulse_terrain_sample(ctypes.byref(s), None) == -1 and b"null out" in err()
    s.out = fake
    assert lib.pulse_terrain_sample(ctypes.byref(s), None) == -1 and b"num_samples must be >= 1" in err()
    s.num_samples = 9
    assert lib.pulse_terrain_sample(ctypes.byref(s), None) == -1 and b"needs coord_x, coord_y and idx" in err()
    s.group_num_people = 24
    assert lib.pulse_terrain_sample(ctypes.byref(s), None) == -1 and b"not a multiple of group_num_people 24" in err()
    s.group_num_people = 16
    assert lib.pulse_terrain_sample(ctypes.byref(s), None) == -1 and b"needs u_center, u_dx and u_dy" in err()
