"""CPU: the 52-body SMPL-X / SMPL-H humanoid below the device.

  * the skeleton descriptions of pulse_amd/synthetic.py (names, tree, dof subset; the SMPL entry is today's constants);
  * oracle/env_oracle.py at 52 bodies against tests/golden/env_smplx.npz, the outputs of the reference's own functions
    (tools/gen_golden_smplx.py): bit for bit -- the oracle is the yardstick of the GPU tests at the new body counts;
  * with the reference checkout present: the generator reproduces the committed fixture key by key;
  * every humanoid / option combination that is not built raises NotImplementedError by name, without a device."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import env_oracle as E
from oracle import refload
from pulse_amd import synthetic as syn
from pulse_amd.env.humanoid_im import check_humanoid_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_golden_smplx", os.path.join(ROOT, "tools", "gen_golden_smplx.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gen():
    return load_generator()


@pytest.fixture(scope="module")
def fixture(gen):
    z = np.load(os.path.join(ROOT, "tests", "golden", "env_smplx.npz"))
    d = gen.inputs()
    for k, v in gen.input_sums(d).items():                    # the redrawn inputs are the ones the fixture was written from
        assert v.item() == z[k].item(), f"{k}: the input recipe draws other numbers than the committed fixture was generated from"
    return z, d


# ------------------------------------------------------------------------------------------------ skeleton descriptions
def test_smplx_skeleton_description():
    sk = syn.SKELETONS["smplx"]
    assert sk is syn.skeleton("smplx") and syn.SKELETONS["smplh"] is sk                # humanoid.py:376: one 52-body skeleton for both
    names, par = sk["body_names"], sk["parents"]
    assert len(names) == 52 and len(set(names)) == 52 and sk["num_bodies"] == 52
    assert sk["num_dof"] == 153
    assert len(sk["dof_subset"]) == 147 and sorted(set(range(153)) - set(sk["dof_subset"])) == [9, 10, 11, 21, 22, 23]
    # a tree rooted at 0 whose parents precede their children (what the forward kinematics of the synthetic library walks)
    assert len(par) == 52 and par[0] == -1 and all(0 <= par[b] < b for b in range(1, 52))
    ix = names.index
    for side in "LR":
        wrist = ix(f"{side}_Wrist")
        assert [names[par[ix(f"{side}_{b}")]] for b in ("Thorax", "Shoulder", "Elbow", "Wrist")] == ["Chest", f"{side}_Thorax", f"{side}_Shoulder", f"{side}_Elbow"]
        for f in ("Index", "Middle", "Pinky", "Ring", "Thumb"):
            assert par[ix(f"{side}_{f}1")] == wrist and par[ix(f"{side}_{f}2")] == ix(f"{side}_{f}1") and par[ix(f"{side}_{f}3")] == ix(f"{side}_{f}2")
    assert names[:18] == syn.SMPL_BODY_NAMES[:18] and par[:18] == syn.SMPL_PARENTS[:18]           # legs, spine and left arm follow the SMPL tree
    assert names[18:33] == ["L_" + f + k for f in ("Index", "Middle", "Pinky", "Ring", "Thumb") for k in "123"]
    assert set(sk["reset_bodies"]) == set(names) - {"L_Ankle", "L_Toe", "R_Ankle", "R_Toe"} and sk["track_bodies"] == names
    assert all(b in names for b in sk["key_bodies"])


def test_smpl_skeleton_is_todays_constants():
    sk = syn.SKELETONS["smpl"]
    assert sk["body_names"] == syn.SMPL_BODY_NAMES and sk["parents"] == syn.SMPL_PARENTS
    assert sk["num_bodies"] == syn.NUM_BODIES == 24 and sk["num_dof"] == syn.NUM_DOF == 69
    assert sk["reset_bodies"] == syn.RESET_BODY_NAMES and sk["track_bodies"] == syn.SMPL_BODY_NAMES
    removed = {syn.SMPL_BODY_NAMES.index(b) - 1 for b in ("L_Hand", "R_Hand", "L_Toe", "R_Toe")}      # humanoid.py:396-421
    assert sk["dof_subset"] == [3 * j + k for j in range(23) if j not in removed for k in range(3)]


def test_synthetic_inputs_take_a_skeleton():
    g = syn.make_generator(3)
    d = syn.env_step_inputs(g, 9, humanoid="smplx")
    assert d["rb"].shape == (9, 52, 13) and d["dof_force"].shape == (9, 153) and d["ref_next"]["rot"].shape == (9, 52, 4)
    a = syn.env_step_inputs(syn.make_generator(3), 9)
    b = syn.env_step_inputs(syn.make_generator(3), 9, humanoid="smpl")
    assert a["rb"].shape == (9, 24, 13) and torch.equal(a["rb"], b["rb"]) and torch.equal(a["dof_vel"], b["dof_vel"])
    tabs = syn.synthetic_motion_library(syn.make_generator(4), 3, 10, 14, humanoid="smplx")
    assert tabs["gts"].shape[1:] == (52, 3) and tabs["lrs"].shape[1:] == (52, 4) and tabs["dvs"].shape[1:] == (51, 3)
    assert torch.allclose(tabs["grs"].norm(dim=-1), torch.ones(()), atol=1e-5)
    # the default is the SMPL library, draw for draw
    t0, t1 = syn.synthetic_motion_library(syn.make_generator(4), 3, 10, 14), syn.synthetic_motion_library(syn.make_generator(4), 3, 10, 14, humanoid="smpl")
    assert all(torch.equal(t0[k], t1[k]) for k in t0)


def test_motion_record_layout_for_52_bodies():
    """The packed frame record MotionLib builds (its host-only layout function): [grs 208 | lrs 208 | gts 156 | gvs 156 | gavs 156 | dvs 153 | pad]
    = 1040 floats at 52 bodies; quaternion fields and the pitch on 16 B at every body count the kernels take."""
    from pulse_amd.env.motion_lib import MotionLib
    offsets, stride, widths = MotionLib.record_layout(52)
    assert offsets == {"grs": 0, "lrs": 208, "gts": 416, "gvs": 572, "gavs": 728, "dvs": 884} and stride == 1040
    assert list(widths.values()) == [208, 208, 156, 156, 156, 153]
    assert MotionLib.record_layout(24)[1] == 480                               # the SMPL record is where it was
    for j in range(1, 65):
        offsets, stride, widths = MotionLib.record_layout(j)
        assert stride % 4 == 0 and offsets["grs"] % 4 == 0 and offsets["lrs"] % 4 == 0
        assert offsets["dvs"] + widths["dvs"] <= stride < offsets["dvs"] + widths["dvs"] + 4
        ends = [offsets[k] + widths[k] for k in widths]
        assert list(offsets.values())[1:] == ends[:-1]                          # fields back to back, none overlapping


# ------------------------------------------------------------------------------------------------ oracle vs the reference's outputs
def _same(got, want, name):
    got = got.numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, name
    assert np.array_equal(got, want), f"{name}: oracle differs from the reference's output (max {np.abs(got - want).max()})"


def test_oracle_equals_reference_outputs_at_52_bodies(fixture, gen):
    z, d = fixture
    rb, rn, rx3 = d["rb"], d["ref_now"], d["ref_next"]
    n = rb.shape[0]
    rx1 = gen.first_sample(rx3, n)
    bp, br, bv, ba = E.split_rb(rb)
    assert z["self_obs"].shape == (n, 778) and z["v6_T1"].shape == (n, 1248) and z["v7_T1_vr"].shape == (n, 27) and z["v6_T3_noup"].shape == (n, 3744)
    tb = gen.TRACK_VR
    for up in (True, False):
        tag = "" if up else "_noup"
        _same(E.self_obs_smpl_max_general(bp, br, bv, ba, upright=up), z["self_obs" + tag], "self_obs" + tag)
        for t, rx in ((1, rx1), (3, rx3)):
            if f"v6_T{t}{tag}" in z.files:
                _same(E.im_obs_variant(6, bp[:, 0], br[:, 0], bp, br, bv, ba, rx["pos"], rx["rot"], rx["vel"], rx["ang"], t, up), z[f"v6_T{t}{tag}"], f"v6_T{t}{tag}")
            sub = lambda x: x[:, tb].contiguous()
            _same(E.im_obs_variant(7, bp[:, 0], br[:, 0], sub(bp), sub(br), sub(bv), sub(ba), sub(rx["pos"]), sub(rx["rot"]), sub(rx["vel"]), sub(rx["ang"]), t, up),
                  z[f"v7_T{t}_vr{tag}"], f"v7_T{t}_vr{tag}")
    _same(E.self_obs_smpl_max(bp, br, bv, ba), z["self_obs"], "self_obs (upright form)")
    _same(E.im_obs_v6(bp[:, 0], br[:, 0], bp, br, bv, ba, rx1["pos"], rx1["rot"], rx1["vel"], rx1["ang"], 1), z["v6_T1"], "im_obs_v6")
    rew, raw = E.im_reward(bp, br, bv, ba, rn["pos"], rn["rot"], rn["vel"], rn["ang"])
    _same(rew, z["reward_im"], "reward_im")
    _same(raw, z["reward_raw_im"], "reward_raw_im")
    rew, raw = E.im_reward_full(rb, rn["pos"], rn["rot"], rn["vel"], rn["ang"], d["dof_force"], d["dof_vel"], d["progress"])
    _same(rew, z["reward"], "reward")
    _same(raw, z["reward_raw"], "reward_raw")
    rid = gen.RESET_IDS
    term_dist = torch.full((1, 52), gen.TERM_DIST)
    for use_mean, tag in ((False, ""), (True, "_mean")):
        reset, term = E.im_reset(torch.zeros(n, dtype=torch.int64), d["progress"], bp[:, rid].clone(), rn["pos"][:, rid].clone(), d["pass_time"],
                                 term_dist[..., rid], use_mean=use_mean)
        _same(reset, z["reset" + tag], "reset" + tag)
        _same(term, z["terminate" + tag], "terminate" + tag)
    # post_physics (what the GPU tests compare against) is these pieces
    pp = E.post_physics(rb, rn, rx1, d["dof_force"], d["dof_vel"], d["progress"], d["pass_time"], rid, list(range(52)), term_dist)
    _same(pp["obs"], np.concatenate([z["self_obs"], z["v6_T1"]], axis=1), "post_physics obs")
    _same(pp["reset"], z["reset"], "post_physics reset")
    _same(pp["terminate"], z["terminate"], "post_physics terminate")


def test_fixture_can_tell_wrong_from_right(fixture, gen):
    z, d = fixture
    rid = gen.RESET_IDS
    dist = torch.norm(d["rb"][:, rid, 0:3] - d["ref_now"]["pos"][:, rid], dim=-1)
    gen.check_conditions(torch.from_numpy(z["reward_raw_im"]), torch.from_numpy(z["terminate"]), torch.cat([dist.flatten(), dist.mean(dim=-1)]))
    share = z["terminate_mean"].astype(np.float64).mean()                              # the use_mean flags are no all-or-nothing answer either
    assert 0.15 <= share <= 0.85, share
    assert np.abs(dist.mean(dim=-1).numpy() - gen.TERM_DIST).min() >= 1e-4
    assert all(z[k].dtype != object for k in z.files)                                   # arrays only


@pytest.mark.skipif(not refload.available(), reason="needs the reference checkout")
def test_oracle_equals_reference_for_the_variant_the_fixture_leaves_out(fixture, gen):
    """v6 over three samples with upright start is not in the fixture (file size); the GPU test holds the kernel to the oracle for it, and
    this holds the oracle to the reference's function."""
    _, d = fixture
    bp, br, bv, ba = E.split_rb(d["rb"])
    rx = d["ref_next"]
    want = gen.reference_v6_three_samples_upright()
    assert want.shape == (d["rb"].shape[0], 3744)
    _same(E.im_obs_variant(6, bp[:, 0], br[:, 0], bp, br, bv, ba, rx["pos"], rx["rot"], rx["vel"], rx["ang"], 3, True), want, "v6_T3")


@pytest.mark.skipif(not refload.available(), reason="needs the reference checkout")
def test_generator_reproduces_committed_fixture(fixture, gen, tmp_path):
    z, _ = fixture
    fresh = gen.generate()
    assert sorted(fresh) == sorted(z.files)
    for k in z.files:
        assert fresh[k].dtype == z[k].dtype and np.array_equal(fresh[k], z[k]), k
    np.savez_compressed(tmp_path / "env_smplx.npz", **fresh)
    assert os.path.getsize(tmp_path / "env_smplx.npz") <= 1024 * 1024


# ------------------------------------------------------------------------------------------------ rejections by name, no device
def test_humanoid_type_is_read_from_the_robot_dict():
    assert check_humanoid_options({"env": {}}) == "smpl"
    assert check_humanoid_options({"env": {}, "robot": {"has_upright_start": True}}) == "smpl"
    assert check_humanoid_options({"env": {"obs_v": 6}, "robot": {"humanoid_type": "smplx", "has_upright_start": False}}) == "smplx"
    assert check_humanoid_options({"env": {"obs_v": 7, "fut_tracks": True}, "robot": {"humanoid_type": "smplh"}}) == "smplh"
    # SMPL keeps every option it has today
    assert check_humanoid_options({"env": {"enable_amp_obs": True, "z_type": "vae", "occl_training": True}, "robot": {"humanoid_type": "smpl"}}) == "smpl"


def test_unknown_humanoid_type_raises_by_name():
    with pytest.raises(NotImplementedError, match="humanoid_type 'g1'"):
        check_humanoid_options({"env": {}, "robot": {"humanoid_type": "g1"}})
    with pytest.raises(NotImplementedError, match="unitree"):
        syn.skeleton("unitree")
    from pulse_amd import configs
    with pytest.raises(NotImplementedError, match="h1"):
        configs.make_env(4, 4, "cuda:0", humanoid="h1")


@pytest.mark.parametrize("ht", ["smplx", "smplh"])
@pytest.mark.parametrize("where,key,value,needle", [
    ("env", "enable_amp_obs", True, "enable_amp_obs"), ("env", "occl_training", True, "occl_training"),
    ("robot", "has_shape_obs", True, "has_shape_obs"), ("robot", "has_weight_obs", True, "has_weight_obs"),
    ("env", "has_shape_obs", True, "has_shape_obs"), ("env", "distill", True, "distill"), ("env", "save_kin_info", True, "distill"),
    ("env", "z_type", "vae", "amp_z"), ("env", "embedding_size", 48, "amp_z")])
def test_unbuilt_smplx_combinations_raise_by_name(ht, where, key, value, needle):
    cfg = {"env": {}, "robot": {"humanoid_type": ht, "has_upright_start": False}}
    cfg[where][key] = value
    with pytest.raises(NotImplementedError, match=needle) as ei:
        check_humanoid_options(cfg)
    assert ht in str(ei.value) and ".py" in str(ei.value)          # names the humanoid and cites the reference lines


def test_unbuilt_smplx_tasks_raise_by_name():
    """HumanoidImGetup and every class of env/humanoid_tasks.py check the humanoid before they touch the simulator or the device."""
    from pulse_amd.env import humanoid_tasks as HT
    from pulse_amd.env.humanoid_im_getup import HumanoidImGetup
    cfg = {"env": {}, "robot": {"humanoid_type": "smplx"}}
    with pytest.raises(NotImplementedError, match="HumanoidImGetup"):
        HumanoidImGetup(cfg, None, None)
    classes = [c for c in vars(HT).values() if isinstance(c, type) and issubclass(c, HT.HumanoidTask)]
    assert len(classes) >= 9
    for cls in classes:
        with pytest.raises(NotImplementedError, match=cls.__name__):
            cls(cfg, None)


def test_amp_z_network_rejects_48_latents_by_name():
    from pulse_amd import configs
    from pulse_amd.learning.network_z import AMPZNetwork
    with pytest.raises(NotImplementedError, match="embedding_size 48"):
        AMPZNetwork(configs.NETWORK_Z, actions_num=153, self_obs_size=778, task_obs_size=1248, task_obs_size_detail={"embedding_size": 48, "z_type": "vae"},
                    device="cpu")


def test_smplx_small_config():
    from pulse_amd import configs
    cfg, n = configs.agent_config("smplx_small")
    assert n == 64 and cfg["horizon_length"] == 16 and cfg["minibatch_size"] == 256 and cfg["network"]["mlp"]["units"] == [512, 512]
    assert cfg["_env_kind"] == "im" and cfg["_agent_kind"] == "common" and cfg["_humanoid"] == "smplx"
    assert configs.ROBOTS["smplx"] == {"humanoid_type": "smplx", "has_upright_start": False}
    assert configs.agent_config("cfg2")[0]["_humanoid"] == "smpl"
