"""CPU: the crowd variant of the terrain task -- the model (tests/crowd_model.py) against the reference's recorded outputs
(tests/golden/crowd.npz, tools/gen_golden_crowd.py), the fixture conditions on the COMMITTED arrays, and the host layers: env keys,
observation widths and detail dicts, the configurations the reference cannot run, the ABI structs, amp_sept's refusals.

Fixture conditions (asserted below, so no kernel error can hide behind an input excuse):
  * among each env's 7 smallest group distances consecutive values differ by more than 1e-4 relative, none is within 1e-4 relative of 10 m
    and no two people coincide: neighbour selection cannot hang on rounding or on topk's tie order;
  * people stand at x, y in [6, 20] m; no sensor sample point and no root point lies within 2e-4 cells of a cell edge (more than 13 fp32
    ulps at those coordinates): heights and stamps must match as indices;
  * footprints of different people of a group occupy disjoint cells in the rows (24, 6), (36, 12) and (160, 80).  In (600, 300) they cannot:
    300 footprints of up to 0.7 m x 1.2 m of cells need 252 m^2 of the 196 m^2 the people of a group share, so that row -- like the
    separately named ``overlap`` scene -- pins the rule that the highest env index owns a shared cell, which is what the reference's indexed
    assignment leaves when it runs serially (the golden is recorded single-threaded for that reason).
"""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

import crowd_model as M
from oracle import refload
from pulse_amd import _lib, configs, synthetic as syn
from pulse_amd.env import env_keys
from pulse_amd.env import humanoid_tasks as HT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "crowd.npz"))
HS = syn.synthetic_height_field()
CASES = M.golden_cases(Z)
SCENES = [M.scene_name(n, g) for n, g in M.SHAPES]


# ---------------------------------------------------------------------------------------------------------------------------- model
@pytest.mark.parametrize("scene", SCENES + ["overlap", "res32"])
def test_model_equals_the_reference_bit_for_bit(scene):
    cases = [c for c in CASES if c["scene"] == scene]
    assert cases
    for c in cases:
        got = M.model_case(c, HS)[c["rows"]]
        assert got.shape == c["ref"].shape, c["key"]
        assert torch.equal(got, c["ref"]), f"{c['key']}: max |diff| {(got - c['ref']).abs().max().item()}"


def test_the_golden_holds_every_kind_switch_and_shape():
    keys = {c["key"] for c in CASES}
    for scene in SCENES:
        for kind in M.KINDS:
            for combo in (M.COMBOS if kind != "group_obs" else M.COMBOS[:2]):
                assert f"{scene}/{kind}/{M.combo_name(*combo)}" in keys
    widths = {c["kind"]: c["ref"].shape[1] for c in CASES if c["scene"] == "n24g6"}
    assert widths == {"group_obs": 64 + 165, "stamps": 64, "stamps_velocity": 192, "velocity": 192}
    assert next(c for c in CASES if c["scene"] == "res32")["ref"].shape == (4, 3 * 1024)
    # the four kinds and the two values of every switch really differ on these inputs
    first = {c["kind"]: c for c in CASES if c["scene"] == "n24g6" and c["key"].endswith(M.combo_name(*M.COMBOS[0]))}
    assert not torch.equal(first["stamps"]["ref"], first["group_obs"]["ref"][:, :64])                   # stamps raise samples
    assert not torch.equal(first["stamps_velocity"]["ref"][:, 1::3], first["velocity"]["ref"][:, 1::3])


@pytest.mark.parametrize("scene", SCENES + ["overlap"])
def test_stamped_cells_equal_the_reference(scene):
    g = M.scene_group_size(scene)
    for rb_key, mask_key in (("rb", "stamped"), ("rb2", "stamped2")):
        if f"{scene}/{rb_key}" not in Z.files:
            continue
        rb = torch.from_numpy(Z[f"{scene}/{rb_key}"])
        own = M.owner_grid(rb, g, *HS.shape)
        assert torch.equal(own > 0, M.stamped_mask(Z, f"{scene}/{mask_key}", own.shape[0]))
        # an owner is a member of the cell's group whose footprint covers it
        cells = M.stamp_cells(rb, *HS.shape)
        for grp in range(own.shape[0]):
            o = own[grp].view(-1)
            idx = o.nonzero().flatten()
            who = o[idx].long() - 1
            assert (who // g == grp).all()
            assert (cells[who] == idx[:, None]).any(dim=1).all()


@pytest.mark.skipif(not refload.available(), reason="the reference tree is not mounted")
def test_golden_regenerates_identically():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_golden_crowd
    fresh = gen_golden_crowd.generate()
    assert sorted(fresh) == sorted(Z.files)
    for k in Z.files:
        assert np.array_equal(fresh[k], Z[k]), k


# ---------------------------------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("n,g", M.SHAPES)
def test_fixture_conditions_hold_on_the_committed_arrays(n, g):
    s = M.scene_name(n, g)
    for key in ("rb", "rb2"):
        rb = torch.from_numpy(Z[f"{s}/{key}"])
        assert rb.shape == (n, 24, 13)
        for name, ok in M.scene_conditions(rb, g, (8,), M.DISJOINT[(n, g)]).items():
            assert ok.all(), f"{s}/{key}: {name} fails for envs {(~ok).nonzero().flatten().tolist()[:8]}"
    rb, rb2 = torch.from_numpy(Z[f"{s}/rb"]), torch.from_numpy(Z[f"{s}/rb2"])
    assert ((rb[:, 0, 0:2] - rb2[:, 0, 0:2]).norm(dim=-1) > 1e-3).all()                   # the second frame: every person moved
    nb, dist = M.neighbours(rb, g)
    assert (nb // g == torch.arange(n)[:, None] // g).all()
    within = (dist <= 10).sum(dim=1).view(-1, g)                                            # per group, per env: neighbours within 10 m
    assert (within[0] == 5).all()                                                           # group 0: nobody is zeroed
    assert ((within > 0) & (within < 5)).any(dim=1).any(), "no group where fewer than 5 people are within 10 m"
    if n // g >= 3:
        assert (within == 0).all(dim=1).any(), "no group where all are beyond 10 m"
    else:
        assert (within[1] == 0).sum() >= g - 4                                              # two groups: the stacked people of group 1 see nobody
    # in the dense group the nearest people OVERALL are mostly in other groups (all groups share the field): a search that ignored the
    # partition would pick them
    p = rb[:, 0, 0:3]
    d = torch.cdist(p[:g].double(), p.double())
    d[torch.arange(g), torch.arange(g)] = float("inf")
    assert (d.argmin(dim=1) >= g).any()
    rows = torch.from_numpy(Z[f"{s}/rows"])
    if len(rows) < n:                                                                       # the subset cuts through every group
        per_group = torch.bincount(rows // g, minlength=n // g)
        assert ((per_group > 0) & (per_group < g)).all()
    if not M.DISJOINT[(n, g)]:
        assert not M._disjoint_ok(rb, g, *HS.shape).all()


def test_fixture_conditions_of_the_overlap_and_32_scenes():
    rb = torch.from_numpy(Z["overlap/rb"])
    for name, ok in M.scene_conditions(rb, 6, (8,), False).items():
        assert ok.all(), name
    assert not M._disjoint_ok(rb, 6, *HS.shape).any()                                       # every footprint shares a cell with another
    own, cells = M.owner_grid(rb, 6, *HS.shape), M.stamp_cells(rb, *HS.shape)
    lost = sum(int((own[e // 6].view(-1)[cells[e]] != e + 1).sum()) for e in range(12))
    assert lost > 100                                                                       # points whose cell a higher index owns
    rb = torch.from_numpy(Z["res32/rb"])
    for name, ok in M.scene_conditions(rb, 6, (8, 32), True).items():
        assert ok.all(), name


# ---------------------------------------------------------------------------------------------------------------------------- host layers
def test_env_keys_accepts_the_crowd_keys():
    keys = ("divide_group", "group_obs", "disable_group_obs", "num_env_group", "velocity_map")
    assert set(keys) <= env_keys.HONOURED and not set(keys) & (set(env_keys.INERT) | set(env_keys.UNBUILT))
    env_keys.audit({"divide_group": True, "group_obs": True, "disable_group_obs": True, "num_env_group": 16, "velocity_map": True}, "test")
    for kind in M.KINDS:
        env_keys.audit(dict(configs.ENV_TERRAIN_Z, **configs.crowd_env(kind, num_env_group=16)), "test")
    assert set(configs.CROWD_ENVS) == set(M.KINDS)


def _task(n=24, cls=HT.HumanoidPedestrianTerrain, **over):
    env = dict(configs.ENV_TERRAIN_Z, sensor_res=8, **over)
    return cls({"env": env}, types.SimpleNamespace(num_envs=n, heightsamples=None), device="cpu")


@pytest.mark.parametrize("key", ["disable_group_obs", "divide_group", "group_obs"])
def test_crowd_options_are_honoured_by_name(key):
    """The successor of tests/test_env_keys.py::test_unbuilt_options_raise_by_name[key] for the three keys that left env_keys.UNBUILT: the
    value that used to raise NotImplementedError naming the key passes the audit, as does the value that was always accepted, and the task
    class ACTS on the key -- switching it alone changes what the task builds."""
    assert key in env_keys.HONOURED and key not in env_keys.UNBUILT and key not in env_keys.INERT
    for value in (True, False):
        env_keys.audit({key: value, "numAMPObsSteps": 10}, "test")
    base = {"divide_group": True, "num_env_group": 6}
    on, off = _task(**dict(base, **{key: True})), _task(**dict(base, **{key: False}))
    if key == "divide_group":                      # groups and stamps exist with it, nothing without it
        assert on._group_num_people == 6 and on._owner is not None and off._group_num_people == 0 and off._owner is None
    elif key == "group_obs":                       # the 'people' block instead of the stamps
        assert "people" in on.get_task_obs_size_detail() and on._owner is None
        assert "people" not in off.get_task_obs_size_detail() and off._owner is not None
    else:                                          # disable_group_obs: groups without stamps (get_heights :749)
        assert on._owner is None and not on._crowd_heights and off._owner is not None and off._crowd_heights
        assert on.get_task_obs_size_detail() == off.get_task_obs_size_detail()


def test_observation_widths_and_detail_dicts():
    base = _task()
    assert base.get_task_obs_size() == 20 + 64 and base.get_task_obs_size_detail() == {"traj": 20, "heightmap": 64}
    assert base._owner is None and not base._crowd_heights and not base._people_obs                    # keys absent: nothing new is allocated
    off = _task(divide_group=False, group_obs=False, velocity_map=False, num_env_group=6)
    assert off.get_task_obs_size_detail() == base.get_task_obs_size_detail() and off._owner is None and off.obs_pitch == base.obs_pitch
    t = _task(**configs.crowd_env("group_obs", num_env_group=6))
    assert t.get_task_obs_size() == 20 + 64 + 165 and t.get_task_obs_size_detail() == {"traj": 20, "heightmap": 64, "people": 165}
    assert list(t.get_task_obs_size_detail()) == ["traj", "heightmap", "people"] and t._owner is None and not t._crowd_heights
    assert t.num_obs == t.get_self_obs_size() + 249
    t = _task(**configs.crowd_env("stamps", num_env_group=6))
    assert t.get_task_obs_size_detail() == {"traj": 20, "heightmap": 64} and t._owner.shape == (4, 260, 300) and t._owner.dtype == torch.int32
    assert t._stamp_cells.shape == (24, 200) and (t._stamp_cells == -1).all()
    t = _task(**configs.crowd_env("stamps_velocity", num_env_group=6))
    assert t.get_task_obs_size() == 20 + 192 and t.get_task_obs_size_detail() == {"traj": 20, "heightmap_velocity": 192} and t._owner is not None
    t = _task(**configs.crowd_env("velocity"))
    assert t.get_task_obs_size_detail() == {"traj": 20, "heightmap_velocity": 192} and t._owner is None and t._crowd_heights
    # group_obs and disable_group_obs switch the stamps off (get_heights :749); the default group size is min(128, num_envs)
    assert _task(divide_group=True, disable_group_obs=True)._owner is None
    assert _task(divide_group=True)._group_num_people == 24 and _task(n=256, divide_group=True)._group_num_people == 128
    # the reference's HumanoidTraj never reads the keys
    t = _task(cls=HT.HumanoidTraj, terrain_obs=False, **configs.crowd_env("group_obs", num_env_group=6))
    assert t.get_task_obs_size_detail() == {"traj": 20}
    # on a plane the heights are zeros before the stamps are looked at: the plain path
    t = _task(terrain={"terrainType": "plane"}, **configs.crowd_env("stamps", num_env_group=6))
    assert t._owner is None and not t._crowd_heights
    cfg, n = configs.agent_config("terrain_z_crowd_small")
    assert n == 64 and cfg["network"]["name"] == "amp_z_reader" and cfg["_env_overrides"] == {"divide_group": True, "group_obs": True, "num_env_group": 16}


def test_configurations_the_reference_cannot_run_raise():
    with pytest.raises(ValueError, match="not a multiple"):
        _task(n=24, divide_group=True, num_env_group=5)
    with pytest.raises(ValueError, match="topk"):
        _task(n=20, divide_group=True, group_obs=True, num_env_group=5)
    _task(n=20, divide_group=True, num_env_group=5)                                        # stamps have no such minimum
    with pytest.raises(NotImplementedError, match="721-725"):
        _task(velocity_map=True, terrain={"terrainType": "plane"})
    with pytest.raises(NotImplementedError, match="fov"):
        _task(terrain_obs_type="fov", divide_group=True)


def test_struct_sizes_match_the_library():
    lib = _lib.load()
    assert lib.pulse_abi_version() == 36
    for cls, fn in ((_lib.CrowdGroupObsArgs, "pulse_sizeof_crowd_group_obs_args"), (_lib.CrowdStampArgs, "pulse_sizeof_crowd_stamp_args"),
                    (_lib.CrowdHeightsArgs, "pulse_sizeof_crowd_heights_args")):
        assert ctypes.sizeof(cls) == getattr(lib, fn)(), fn
    assert (_lib.CROWD_GROUP_OBS, _lib.CROWD_ROOT_POINTS) == (M.GROUP_OBS, M.ROOT_POINTS)


def test_amp_sept_says_why_it_refuses_the_crowd_observations():
    from pulse_amd.learning.network_sept import AMPSeptNetwork
    kw = dict(actions_num=32, self_obs_size=358, device="cpu")
    with pytest.raises(NotImplementedError, match=r"amp_network_sept_builder.py:48-60.*amp_z_reader"):
        AMPSeptNetwork(configs.NETWORK_SEPT, task_obs_size=249, task_obs_size_detail={"traj": 20, "heightmap": 64, "people": 165}, **kw)
    with pytest.raises(ValueError, match=r"heightmap_velocity.*amp_network_sept_builder.py:107"):
        AMPSeptNetwork(configs.NETWORK_SEPT, task_obs_size=212, task_obs_size_detail={"traj": 20, "heightmap_velocity": 192}, **kw)
