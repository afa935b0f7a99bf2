"""CPU: the reference-state reset of the downstream tasks.

  * tests/task_reset_model.py (what tests/test_task_reset_gpu.py measures pulse_task_ref_state_init against) pinned to the reference's own
    _sample_ref_state / _reset_ref_state_init bodies of HumanoidAMP, HumanoidSpeed, HumanoidReach, HumanoidStrike and
    HumanoidPedestrianTerrain: extracted by name (oracle/refload.py), rebuilt as a class chain so that their ``super()`` calls resolve, run
    on stubs.  Root state, dofs, ids, times and the transient _rigid_body_* cache bit for bit; and the three documented places where the
    rigidly carried bodies the kernel writes differ from that cache, and nothing else.  Live, the reference code runs; replayed, its values
    come from tests/golden/ref/test_task_reset_cpu/.  _get_fixed_smpl_state_from_motionlib (SMPL mesh parsers: fix_trans_height) is stubbed
    by the motion's own state: out of scope, as for MotionLib.
  * what the new env options reject by name, the SyntheticTaskSim default, the new configs.
"""
import enum
import os
import textwrap
import types

import pytest
import torch

import task_reset_model as M
from amp_frame_model import non_upright_tables
from oracle import refload
from oracle.motion_oracle import OracleMotionLib
from oracle.refrecord import RefRecord
from pulse_amd import configs, synthetic as syn
from pulse_amd.env import humanoid_tasks as HT

N = 12
HSCALE, VSCALE = 0.1, 0.005
CASES = [("HumanoidAMP", "none", True), ("HumanoidReach", "zero_xy", True), ("HumanoidStrike", "zero_xy", True),
         ("HumanoidSpeed", "remove_heading", True), ("HumanoidSpeed", "remove_heading", False), ("HumanoidPedestrianTerrain", "terrain", True)]


class StateInit(enum.Enum):
    Default, Start, Random, Hybrid = 0, 1, 2, 3


class _Stub:
    """What the extracted methods reach for beside each other: the library's draws, the SMPL height fix (out of scope: the motion's own
    state), and the simulator hand-over, which is recorded."""

    def _get_fixed_smpl_state_from_motionlib(self, motion_ids, motion_times, curr_gender_betas):
        r = self._motion_lib.get_motion_state(motion_ids, motion_times)
        return (r["root_pos"], r["root_rot"], r["dof_pos"], r["root_vel"], r["root_ang_vel"], r["dof_vel"], r["rg_pos"], r["rb_rot"], r["body_vel"],
                r["body_ang_vel"])

    def _set_env_state(self, **kw):
        self.handed = {k: v.clone() for k, v in kw.items() if isinstance(v, torch.Tensor)}


def _reference_classes():
    """The five classes' reset methods as a class chain (text read from the reference checkout at run time)."""
    T = refload.terrain_functions()
    ns = refload._namespace()
    base_rot = refload.env_functions()["remove_base_rot"]
    ns.update({"_Stub": _Stub, "flags": types.SimpleNamespace(follow=False, fixed=False, server_mode=False), "remove_base_rot": base_rot,
               "humanoid_amp": types.SimpleNamespace(remove_base_rot=base_rot), "quat_apply_yaw": T["quat_apply_yaw"]})
    tasks = os.path.join(refload.REFERENCE_ROOT, "phc", "env", "tasks")
    for cls, fname, names, base in (("HumanoidAMP", "humanoid_amp.py", ["_sample_ref_state", "_reset_ref_state_init", "_sample_time"], "_Stub"),
                                    ("HumanoidSpeed", "humanoid_speed.py", ["_sample_ref_state", "_reset_ref_state_init"], "HumanoidAMP"),
                                    ("HumanoidReach", "humanoid_reach.py", ["_sample_ref_state"], "HumanoidAMP"),
                                    ("HumanoidStrike", "humanoid_strike.py", ["_sample_ref_state"], "HumanoidAMP"),
                                    ("HumanoidPedestrianTerrain", "humanoid_pedestrian_terrain.py",
                                     ["_sample_ref_state", "_reset_ref_state_init", "get_center_heights"], "HumanoidAMP")):
        srcs = refload._extract(os.path.join(tasks, fname), names, methods_of=cls)
        text = f"class {cls}({base}):\n" + "\n".join(textwrap.indent(srcs[k], "    ") for k in names)
        exec(compile(text, f"<reference:{cls}>", "exec"), ns)
    ns["HumanoidAMP"].StateInit = StateInit
    return ns, T


def _inputs(upright):
    g = syn.make_generator(41)
    tabs = syn.synthetic_motion_library(g, 5, 12, 30)
    if not upright:
        tabs = non_upright_tables(tabs)
    lib = OracleMotionLib(tabs)
    ids = torch.randint(0, 5, (N,), generator=g)
    times = torch.rand(N, generator=g) * tabs["motion_lengths"][ids]
    times[0], times[1], times[2] = 0.0, tabs["motion_lengths"][ids[1]], tabs["motion_lengths"][ids[2]] + 0.7      # start, exact length, past the end
    hs, cp = syn.synthetic_height_field(), torch.cat([syn.center_height_points(), torch.zeros(9, 1)], dim=1)
    xy = 3.0 + torch.rand(N, 2, generator=g) * torch.tensor([20.0, 24.0])
    return lib, ids, times, hs, cp, xy


def _run_reference(cls_name, upright, lib, ids, times, hs, cp, xy):
    ns, T = _reference_classes()
    me = ns[cls_name].__new__(ns[cls_name])
    terrain = refload.stub_self(heightsamples=hs, horizontal_scale=HSCALE, vertical_scale=VSCALE, sample_valid_locations=lambda n, env_ids: xy.clone())
    terrain.world_points_to_map = lambda pts: T["Terrain.world_points_to_map"](terrain, pts)
    terrain.sample_height_points = lambda pts, **kw: T["Terrain.sample_height_points"](terrain, pts, **kw)
    motion_lib = refload.stub_self(sample_motions=lambda n: ids.clone(), sample_time_interval=lambda m: times.clone(), get_motion_state=lib.get_motion_state)
    me.__dict__.update(_motion_lib=motion_lib, _state_init=StateInit.Random, humanoid_type="smpl", humanoid_shapes=torch.zeros(N, 17), device="cpu",
                       _has_upright_start=upright, _body_names=list(syn.SMPL_BODY_NAMES), _key_body_ids=torch.tensor([7, 3, 18, 23]), num_envs=N,
                       power_acc=torch.ones(N, 2), _motion_start_times=torch.full((N,), -1.0), _sampled_motion_ids=torch.full((N,), -1, dtype=torch.int64),
                       terrain=terrain, big_ankle=False, cfg={"env": {"terrain": {"terrainType": "trimesh"}}}, num_center_height_points=9,
                       center_height_points=cp[None].repeat(N, 1, 1))
    me._reset_ref_state_init(torch.arange(N))
    return me


@pytest.mark.parametrize("cls_name,transform,upright", CASES, ids=[f"{c}-{'up' if u else 'noup'}" for c, _, u in CASES])
def test_model_matches_reference_methods(request, cls_name, transform, upright):
    rec = RefRecord(request)
    lib, ids, times, hs, cp, xy = _inputs(upright)
    if transform == "remove_heading":
        assert M.heading_axis_xy(lib, ids, times, upright).min() >= 0.1          # the heading is atan2 of this projection
    me = _run_reference(cls_name, upright, lib, ids, times, hs, cp, xy) if rec.live else None
    m = M.ref_state(lib, ids, times, transform, upright=upright, new_root_xy=xy, heightsamples=hs, center_points=cp, horizontal_scale=HSCALE,
                    vertical_scale=VSCALE)
    # ---- what the reference hands to the simulator, and what it keeps: bit for bit
    for key, handed in (("root_pos", "root_pos"), ("root_rot", "root_rot"), ("root_vel", "root_vel"), ("root_ang_vel", "root_ang_vel"),
                        ("dof_pos", "dof_pos"), ("dof_vel", "dof_vel")):
        assert rec.equal(m[key], rec.t(key, lambda: me.handed[handed])), key
    assert torch.equal(m["motion_ids"], rec.t("ids", lambda: me._reset_ref_motion_ids))
    assert rec.equal(m["motion_times"], rec.t("times", lambda: me._reset_ref_motion_times))
    if cls_name != "HumanoidPedestrianTerrain":      # (its _reset_ref_state_init leaves the two per-env tensors alone, :583-585)
        assert torch.equal(m["motion_ids"], rec.t("sampled_ids", lambda: me._sampled_motion_ids))
        assert rec.equal(m["motion_times"], rec.t("start_times", lambda: me._motion_start_times))
    if cls_name == "HumanoidSpeed":
        assert (rec.t("power_acc", lambda: me.power_acc) == 0).all()
    for key, handed in (("rb_pos", "rigid_body_pos"), ("rb_rot", "rigid_body_rot"), ("body_vel", "rigid_body_vel"), ("body_ang_vel", "rigid_body_ang_vel")):
        assert rec.equal(m["cache"][key], rec.t("cache/" + key, lambda: me.handed[handed])), key
    rec.close()
    # ---- the records: body 0 is that root state ...
    r, c, mo = m["records"], m["cache"], m["motion"]
    assert torch.equal(r[:, 0], torch.cat([m["root_pos"], m["root_rot"], m["root_vel"], m["root_ang_vel"]], dim=-1))
    # ... and the other bodies equal the reference's cache except in the documented place of each task
    pos, rot, vel, ang = r[:, 1:, 0:3], r[:, 1:, 3:7], r[:, 1:, 7:10], r[:, 1:, 10:13]
    assert torch.equal(rot, c["rb_rot"][:, 1:]) and torch.equal(vel, c["body_vel"][:, 1:])
    if transform == "remove_heading":            # body_ang_vel is returned unrotated (humanoid_speed.py:262-270)
        assert torch.equal(pos, c["rb_pos"][:, 1:])
        assert torch.equal(c["body_ang_vel"], mo["body_ang_vel"]) and not torch.equal(ang, c["body_ang_vel"][:, 1:])
        assert (ang.norm(dim=-1) - mo["body_ang_vel"][:, 1:].norm(dim=-1)).abs().max() < 1e-4          # the same vectors, turned
    elif transform == "zero_xy":                 # the bodies are not translated with the root (humanoid_reach.py:46-49)
        assert torch.equal(ang, c["body_ang_vel"][:, 1:]) and torch.equal(c["rb_pos"], mo["rb_pos"])
        assert torch.equal(pos[..., 2], c["rb_pos"][:, 1:, 2]) and torch.equal(pos[..., 0:2], c["rb_pos"][:, 1:, 0:2] - mo["rb_pos"][:, :1, 0:2])
        assert (mo["rb_pos"][:, 0, 0:2].abs() > 1e-3).any()
    elif transform == "terrain":                 # moved in xy but never lifted (humanoid_pedestrian_terrain.py:563-567)
        assert torch.equal(ang, c["body_ang_vel"][:, 1:]) and torch.equal(pos[..., 0:2], c["rb_pos"][:, 1:, 0:2])
        assert torch.equal(pos[..., 2], c["rb_pos"][:, 1:, 2] + m["center_height"][:, None]) and (m["center_height"].abs() > 1e-3).any()
    else:
        assert torch.equal(pos, c["rb_pos"][:, 1:]) and torch.equal(ang, c["body_ang_vel"][:, 1:])


# ------------------------------------------------------------------------------------------------------------------ options, sim, configs
def _task(env, motion_lib=None, cls=HT.HumanoidSpeed, robot=None):
    sim = HT.SyntheticTaskSim(4, 2, "cpu")
    cfg = {"env": env} if robot is None else {"env": env, "robot": robot}
    return cls(cfg, sim, device="cpu", motion_lib=motion_lib)


def test_amp_layer_rejections_by_name():
    lib = types.SimpleNamespace(num_bodies=24)
    with pytest.raises(ValueError, match=r"enable_amp_obs.*motion_lib"):
        _task({"enable_amp_obs": True})
    for state_init in ("Hybrid", "Default"):
        with pytest.raises(NotImplementedError, match=rf"stateInit '{state_init}'.*humanoid_amp\.py:447-505"):
            _task({"enable_amp_obs": True, "stateInit": state_init}, lib)
    for key in ("has_shape_obs_disc", "has_weight_obs_disc"):
        with pytest.raises(NotImplementedError, match=key):
            _task({"enable_amp_obs": True, key: True}, lib, cls=HT.HumanoidReach)
        with pytest.raises(NotImplementedError, match=key):
            _task({"enable_amp_obs": True}, lib, cls=HT.HumanoidPedestrianTerrain, robot={"humanoid_type": "smpl", key: True})
    # the switch off: none of this is looked at, and no AMP window exists
    task = _task({"stateInit": "Hybrid"})
    assert task._enable_amp_obs is False and not hasattr(task, "_amp")


def test_synthetic_task_sim_default_is_unchanged():
    a, b = HT.SyntheticTaskSim(5, 3, "cpu", seed=9), HT.SyntheticTaskSim(5, 3, "cpu", seed=9, dof_pos_bank=False)
    c = HT.SyntheticTaskSim(5, 3, "cpu", seed=9, dof_pos_bank=True)
    assert sorted(a.bank) == sorted(b.bank) and "dof_pos" not in a.bank
    for other in (b, c):
        for k in a.bank:
            assert torch.equal(a.bank[k], other.bank[k]), k
        for k in ("rigid_body_state", "contact_forces", "dof_force", "dof_vel", "target_states", "target_contact_forces"):
            assert torch.equal(getattr(a, k), getattr(other, k)), k
    assert torch.equal(a.dof_pos, b.dof_pos) and (a.dof_pos == 0).all()
    assert c.bank["dof_pos"].shape == (3, 5, 69) and torch.equal(c.dof_pos, c.bank["dof_pos"][0])
    c.simulate_and_refresh()
    a.simulate_and_refresh()
    assert torch.equal(c.dof_pos, c.bank["dof_pos"][1]) and torch.equal(c.rigid_body_state, a.rigid_body_state) and (a.dof_pos == 0).all()
    assert c.set_env_states_masked(torch.ones(5, dtype=torch.bool)) is None


@pytest.mark.parametrize("name,network", [("speed_z_amp_small", "amp_z_reader"), ("terrain_z_amp_small", "amp_sept")])
def test_amp_task_configs(name, network):
    cfg, num_envs = configs.agent_config(name)
    assert num_envs == 64 and cfg["horizon_length"] == 16 and cfg["minibatch_size"] == 256
    assert cfg["network"]["name"] == network and cfg["network"]["mlp"]["units"] == [256, 128] and cfg["network"]["disc"]["units"] == [1024, 512]
    assert cfg["_env_overrides"] == {"enable_amp_obs": True, "numAMPObsSteps": 10}
    assert cfg["task_reward_w"] == 1 and cfg["disc_reward_w"] == 0 and cfg["disc_coef"] == 5 and cfg["grad_norm"] == 50.0     # pulse_z_task.yaml:90-91
    small = configs.agent_config("cfg5_small")[0]
    for k in ("amp_minibatch_size", "amp_obs_demo_buffer_size", "amp_replay_buffer_size", "amp_batch_size"):
        assert cfg[k] == small[k], k
    assert cfg["_agent_kind"] == "amp" and "enable_disc" not in cfg          # the discriminator follows the env's amp_observation_space


def test_reset_entry_point_binding():
    """The new struct as the C compiler lays it out, the transform codes of the header, and the argument errors that need no device."""
    import ctypes
    import re
    from pulse_amd import _lib, ops
    lib = _lib.load()
    assert ctypes.sizeof(_lib.TaskResetArgs) == lib.pulse_sizeof_task_reset_args()
    assert lib.pulse_abi_version() == 36                                     # an added entry point: no existing struct or signature changed
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pulse_hip.h")).read()
    codes = {k.lower(): int(v) for k, v in re.findall(r"#define PULSE_TASK_RESET_([A-Z_]+) (\d+)", header)}
    assert codes == ops.TASK_RESET_TRANSFORMS and len(codes) == 4
    assert lib.pulse_task_ref_state_init(None, None) == -1 and b"null args" in lib.pulse_last_error()
    a = _lib.TaskResetArgs()
    a.tab.num_bodies, a.num_envs = 33, 4
    assert lib.pulse_task_ref_state_init(ctypes.byref(a), None) == -1 and b"num_bodies 33 not in [2,32]" in lib.pulse_last_error()
    a.tab.num_bodies, a.num_envs = 24, 0
    assert lib.pulse_task_ref_state_init(ctypes.byref(a), None) == 0          # zero envs: nothing to do


def test_amp_seed_is_a_key_of_the_package():
    from pulse_amd.env import env_keys
    assert "amp_seed" in env_keys.HONOURED
