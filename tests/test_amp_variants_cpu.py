"""CPU: the AMP frame's configured variants -- discriminator shape / limb rows, non-upright root, amp_obs_v 2.

  * the width entry (pulse_amp_obs_width_v) against _num_amp_obs_per_step of the reference (humanoid_amp.py:296-314) for every combination;
  * the option errors that need no device: amp_obs_v 2 + has_shape_obs_disc, amp_obs_v 3, a motion library without shape rows;
  * the env_keys classification of amp_obs_v / has_shape_obs_disc / has_weight_obs_disc;
  * tests/amp_frame_model.py (the restatement the GPU tests measure the kernels against) held to tests/golden/env_amp_variants.npz -- written
    by the reference's own build_amp_observations_smpl / _v2 -- bit for bit, and the generator reproducing the fixture where the reference
    is present;
  * HumanoidAMP's own _compute_amp_observations / _update_hist_amp_obs / _init_amp_obs bodies on a stub with _has_shape_obs_disc True,
    _has_upright_start False (and once amp_obs_v 2) against the restatement's window, over a reset, three steps and a partial reset.
"""
import importlib.util
import itertools
import os
import types
import warnings

import numpy as np
import pytest
import torch

import amp_frame_model as M
from oracle import refload
from oracle.motion_oracle import OracleMotionLib
from oracle.refrecord import RefRecord
from pulse_amd import ops, synthetic as syn
from pulse_amd.env import env_keys as K
from pulse_amd.env.humanoid_im import check_amp_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_golden_amp_variants", os.path.join(ROOT, "tools", "gen_golden_amp_variants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gen():
    return load_generator()


@pytest.fixture(scope="module")
def fixture(gen):
    z = gen.load()
    d = gen.inputs()
    for k, v in gen.input_sums(d).items():                    # the redrawn inputs are the ones the fixture was written from
        assert v.item() == z[k].item(), f"{k}: the input recipe draws other numbers than the committed fixture was generated from"
    return z, d


def model_frame(gen, d, spec):
    return M.frame_from_records(d["rb"], d["dof_pos"], d["dof_vel"], gen.KEY, d["shapes"][:, :-6] if spec["shape"] else None,
                                d["limbs"] if spec["limb"] else None, dof_subset=torch.tensor(gen.SUBSET) if spec["subset"] else None,
                                root_height_obs=spec["height"], upright=spec["upright"], version=spec["version"])


# ------------------------------------------------------------------------------------------------ width
def test_width_entry_matches_the_reference_formula():
    seen = {}
    for version, height, subset, shape, limb in itertools.product((1, 2), (True, False), (True, False), (True, False), (True, False)):
        nj = 19 if subset else 23
        want = M.frame_width(23, 4, height, version, subset, shape, limb)
        got = ops.amp_obs_width(nj, 4, height, version=version, num_shape=11 * shape, num_limb=10 * limb)
        assert got == want, (version, height, subset, shape, limb, got, want)
        seen[(version, height, subset, shape, limb)] = got
    assert seen[(1, True, True, False, False)] == 196 and seen[(1, True, True, True, False)] == 207       # shipped; shipped shape-aware
    assert seen[(2, True, True, False, False)] == 208 and seen[(1, True, True, True, True)] == 217
    assert seen[(1, True, False, False, False)] == 232 and seen[(2, True, False, False, False)] == 244
    assert max(seen.values()) == 265 <= 320                                                               # inside amp_obs.hip's kAmpMaxW
    # the three-argument entry keeps its meaning
    assert ops.amp_obs_width(23, 4) == 232 and ops.amp_obs_width(19, 4, False) == 195
    with pytest.raises(ValueError, match="version"):
        ops.amp_obs_width(23, 4, version=3)


# ------------------------------------------------------------------------------------------------ option errors
def test_option_errors_name_their_keys():
    amp = {"enable_amp_obs": True}
    assert check_amp_options(dict(amp)) == 1 and check_amp_options(dict(amp, amp_obs_v=2, has_weight_obs_disc=True)) == 2
    with pytest.raises(NotImplementedError, match=r"amp_obs_v 2 with has_shape_obs_disc.*humanoid_amp\.py:675.*humanoid_amp\.py:312"):
        check_amp_options(dict(amp, amp_obs_v=2, has_shape_obs_disc=True))
    with pytest.raises(ValueError, match="amp_obs_v = 3"):
        check_amp_options(dict(amp, amp_obs_v=3))
    bare = types.SimpleNamespace(query=None, motion_bodies=None, motion_limb_weights=None)
    with pytest.raises(ValueError, match="has_shape_obs_disc: the motion library carries no motion_bodies"):
        check_amp_options(dict(amp, has_shape_obs_disc=True), bare)
    with pytest.raises(ValueError, match="has_weight_obs_disc: the motion library carries no motion_limb_weights"):
        check_amp_options(dict(amp, has_weight_obs_disc=True), bare)
    full = types.SimpleNamespace(query=None, motion_bodies=torch.zeros(2, 17), motion_limb_weights=torch.zeros(2, 10))
    check_amp_options(dict(amp, has_shape_obs_disc=True, has_weight_obs_disc=True), full)
    recorded = types.SimpleNamespace()                                                # recorded frames: no motions, the envs' own rows
    check_amp_options(dict(amp, has_shape_obs_disc=True), recorded)


def test_synthetic_library_shape_rows_leave_the_tables_alone():
    a = syn.synthetic_motion_library(syn.make_generator(4), 5, 10, 14)
    b = syn.synthetic_motion_library(syn.make_generator(4), 5, 10, 14, shape_rows=True)
    assert "motion_bodies" not in a and set(b) - set(a) == {"motion_bodies", "motion_limb_weights"}
    assert all(torch.equal(a[k], b[k]) for k in a)                                    # draw for draw
    assert b["motion_bodies"].shape == (5, 17) and b["motion_limb_weights"].shape == (5, 10)
    for t in (b["motion_bodies"], b["motion_limb_weights"]):
        assert (t.max(dim=0).values > t.min(dim=0).values).all()                      # no constant column


# ------------------------------------------------------------------------------------------------ env keys
def test_env_keys_classification():
    for k in ("has_shape_obs_disc", "has_weight_obs_disc"):
        assert k in K.HONOURED and k not in K.UNBUILT and k not in K.INERT
    for k in ("remove_disc_rot", "numAMPEncObsSteps", "enableHistObs"):
        assert k in K.UNBUILT
    # amp_obs_v 2 is accepted where the AMP frame is built, and still raises by name where it would be dropped (no AMP observation in the env)
    assert "amp_obs_v" in K.UNBUILT and "amp_obs_v" not in K.HONOURED
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                               # none of the three is reported as unread any more
        K.audit({"enable_amp_obs": True, "amp_obs_v": 2, "has_shape_obs_disc": True, "has_weight_obs_disc": True}, "test")
        K.audit({"amp_obs_v": 1}, "test")
    with pytest.raises(NotImplementedError, match="amp_obs_v"):
        K.audit({"amp_obs_v": 2}, "test")
    with pytest.raises(NotImplementedError, match="amp_obs_v"):
        K.audit({"enable_amp_obs": False, "amp_obs_v": 2}, "test")


# ------------------------------------------------------------------------------------------------ restatement vs fixture
def test_restatement_matches_the_fixture_bit_for_bit(gen, fixture):
    z, d = fixture
    assert len(gen.VARIANTS) == 14
    for name, spec in gen.VARIANTS.items():
        got = model_frame(gen, d, spec).numpy()
        assert got.shape == z[name].shape == (gen.N, gen.columns(spec)["width"]), name
        assert np.array_equal(got, z[name]), f"{name}: the restatement differs from the reference's output"
    gen.check_conditions({k: torch.from_numpy(z[k]) for k in gen.VARIANTS})


@pytest.mark.skipif(not refload.available(), reason="needs the reference checkout")
def test_generator_reproduces_the_committed_fixture(gen):
    z = np.load(os.path.join(ROOT, "tests", "golden", "env_amp_variants.npz"))
    new = gen.generate()
    assert set(new) == set(z.files)
    for k in z.files:
        assert new[k].dtype == z[k].dtype and np.array_equal(new[k], z[k]), k
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "env_amp_variants.npz")) < gen.MAX_BYTES


# ------------------------------------------------------------------------------------------------ window vs the reference's methods
def _ref_motion_lib(tabs):
    lib = refload.motion_lib_class()()
    for k in ("gts", "grs", "lrs", "gvs", "gavs", "dvs", "length_starts"):
        setattr(lib, k, tabs[k])
    lib._motion_lengths, lib._motion_fps, lib._motion_dt = tabs["motion_lengths"], tabs["motion_fps"], tabs["motion_dt"]
    lib._motion_num_frames, lib.num_bodies, lib._device = tabs["motion_num_frames"], syn.NUM_BODIES, "cpu"
    lib._motion_aa = torch.zeros(tabs["gts"].shape[0], 72)
    lib._motion_bodies, lib._motion_limb_weights = tabs["motion_bodies"], tabs["motion_limb_weights"]
    return lib


class _OverlapChecked:
    """The history view with the partial-overlap check of the PyTorch the reference targets (`hist[:] = buf[:, 0:S-1]` raises there and
    _update_hist_amp_obs falls back to its `.clone()` form, humanoid_amp.py:624-627); see tests/test_oracle_env_vs_reference_methods.py."""

    def __init__(self, view, whole):
        self.view, self.whole = view, whole

    def __setitem__(self, idx, val):
        lo, hi = self.whole.data_ptr(), self.whole.data_ptr() + self.whole.numel() * 4
        if isinstance(val, torch.Tensor) and lo <= val.data_ptr() < hi:
            raise RuntimeError("unsupported operation: some elements of the input tensor and the written-to tensor refer to a single memory location")
        self.view[idx] = val

    def __getitem__(self, idx):
        return self.view[idx]


@pytest.mark.parametrize("variant", ["shape_limb_noup_v1", "limb_noup_v2"])
def test_amp_window_variants_match_reference_methods(request, gen, variant):
    """AmpWindow vs HumanoidAMP's own method bodies on a stub: shape + limb rows, non-upright (v1); limb rows, non-upright, amp_obs_v 2
    (v2 with the shape row cannot run in the reference: humanoid_amp.py:312 vs :675)."""
    version = 2 if variant.endswith("v2") else 1
    shape_disc = version == 1
    R = RefRecord(request)
    f = dict(refload.humanoid_amp_methods()) if R.live else {}
    if R.live and version == 2:              # the v2 jit function is not in refload's table: read beside it, made visible to the method bodies
        f["_compute_amp_observations_from_state"].__globals__["build_amp_observations_smpl_v2"] = gen.reference_functions()["build_amp_observations_smpl_v2"]
    n, S, dt = 21, 10, 2.0 / 60.0
    g = syn.make_generator(8)
    tabs = syn.synthetic_motion_library(g, n, 10, 24, shape_rows=True)
    lib = _ref_motion_lib(tabs) if R.live else None
    key = torch.tensor(gen.KEY)
    subset = torch.tensor(gen.SUBSET)
    shapes = torch.cat([torch.randint(0, 2, (n, 1), generator=g).float(), torch.randn(n, 16, generator=g)], dim=1)
    limbs = torch.rand(n, 10, generator=g) + 0.5
    W = M.frame_width(23, 4, True, version, True, shape_disc, True)
    assert W == (217 if version == 1 else 218)
    twin = M.AmpWindow(OracleMotionLib(tabs), torch.arange(n), S, dt, key, dof_subset=subset, shapes=shapes, limbs=limbs,
                       motion_bodies=tabs["motion_bodies"], motion_limb_weights=tabs["motion_limb_weights"], has_shape_obs_disc=shape_disc,
                       has_limb_weight_obs_disc=True, upright=False, version=version)
    amp_buf = torch.zeros(n, S, W)
    task = types.SimpleNamespace(
        humanoid_type="smpl", dof_subset=subset, _amp_obs_buf=amp_buf, _curr_amp_obs_buf=amp_buf[:, 0], _hist_amp_obs_buf=_OverlapChecked(amp_buf[:, 1:], amp_buf),
        _num_amp_obs_steps=S, dt=dt, device="cpu", _key_body_ids=key, _local_root_obs=True, _amp_root_height_obs=True, _has_dof_subset=True,
        _has_shape_obs_disc=shape_disc, _has_limb_weight_obs_disc=True, _has_upright_start=False, amp_obs_v=version, humanoid_shapes=shapes,
        humanoid_limb_and_weights=limbs, _motion_lib=lib, ref_motion_cache={}, gym=None, sim=None)
    for k, fn in f.items():
        setattr(task, k, types.MethodType(fn, task))
    starts = OracleMotionLib(tabs).sample_time_interval(torch.arange(n), generator=g)
    for step in range(5):                                                      # a reset, three steps, a partial reset
        rb = syn.rigid_body_state(g, n)
        dp, dv = 0.5 * torch.randn(n, 69, generator=g), torch.randn(n, 69, generator=g)
        if R.live:
            task._rigid_body_pos, task._rigid_body_rot, task._rigid_body_vel, task._rigid_body_ang_vel = rb[..., 0:3], rb[..., 3:7], rb[..., 7:10], rb[..., 10:13]
            task._dof_pos, task._dof_vel = dp.clone(), dv.clone()
        env_ids = torch.arange(n) if step == 0 else torch.tensor([1, 4, 5, 17]) if step == 4 else None
        if step == 4:
            starts = OracleMotionLib(tabs).sample_time_interval(torch.arange(n), generator=g)
        if env_ids is not None:                                                # _init_amp_obs with reference-state init
            if R.live:
                task._reset_default_env_ids, task._reset_ref_env_ids = [], env_ids
                task._reset_ref_motion_ids, task._reset_ref_motion_times = torch.arange(n)[env_ids], starts[env_ids]
                task._init_amp_obs(env_ids)
            twin.reset(env_ids, rb, dp, dv, starts, from_motion=True)
        else:                                                                  # HumanoidAMP.post_physics_step (:194-210)
            if R.live:
                task._update_hist_amp_obs()
                task._compute_amp_observations()
            twin.step(rb, dp, dv)
        assert R.matches(f"amp_buf/{step}", lambda: amp_buf, twin.buf), f"step {step}"
    # the rows really are in the window: the env's in slot 0, the motion's in the history of a reset env
    assert torch.equal(twin.buf[:, 0, -10:], limbs) and torch.equal(twin.buf[4, 1, -10:], tabs["motion_limb_weights"][4])
    if shape_disc:
        assert torch.equal(twin.buf[:, 0, -21:-10], shapes[:, :11]) and torch.equal(twin.buf[4, 5, -21:-10], tabs["motion_bodies"][4, :11])
    # default init (no motion to look back into): the history repeats the first frame, rows included
    ids = torch.tensor([0, 2, 9])
    if R.live:
        task._reset_default_env_ids, task._reset_ref_env_ids = ids, []
        task._init_amp_obs(ids)
    twin.reset(ids, rb, dp, dv, starts, from_motion=False)
    assert R.matches("amp_buf/default", lambda: amp_buf, twin.buf)
    R.close()
