"""CPU: the yardsticks pulse_motion_ingest is held to, and everything of the feature that needs no device.

  * tests/motion_ingest_model.py (the fp64 numpy restatement the GPU tests also use) agrees with tests/golden/motion_ingest.npz -- the outputs of
    the reference's two conversion scripts, tools/gen_golden_motion_ingest.py -- to fp64 rounding, signs included; the same agreement is
    checked against the scripts' statements run live where the reference checkout is present (RefRecord), and replayed from
    tests/golden/ref/ elsewhere;
  * on the committed arrays, every quaternion whose sign the reference decides (the un-normalised quat_mul products down the tree and
    back, and the normalised outputs made from them) has |w| >= the fixture's floor, 1e-3 -- more than a thousand times the 6.9e-7 the GPU
    test allows a component to be off, so no sign can flip within fp32 rounding.  Nothing is masked;
  * the fixture's cases are the ones the generator describes, and a fresh run reproduces it where the reference is present;
  * the entry point's struct as the C compiler lays it out, the ABI version, and every message of the launcher's argument checks;
  * the host logic of MotionLib.from_smpl_data: key order, dropped clips, mirror keys, both spellings of the input keys."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden_motion_ingest as GI  # noqa: E402
import motion_ingest_model as MI  # noqa: E402
from oracle import refload  # noqa: E402
from oracle.refrecord import RefRecord  # noqa: E402
from pulse_amd import _lib  # noqa: E402
from pulse_amd import synthetic as syn  # noqa: E402
from pulse_amd.env import motion_lib as ML  # noqa: E402

FP64_ROUNDING = 1e-14          # a few dozen fp64 operations on unit quaternions and metre-sized translations
INVALID = -1


@pytest.fixture(scope="module")
def fx():
    return GI.load()


def model(fx, clip, **kw):
    return MI.ingest_clip(clip["poses"], clip["trans"], clip["framerate"], syn.SMPL_PARENTS, syn.smpl_joint_map(), bound=clip["bound"],
                          root_offset=fx["root_offset"], mirror_map=syn.mirror_body_map(), **kw)


def agrees(got, want):
    return got.shape == want.shape and np.array_equal(np.signbit(got), np.signbit(want)) and float(np.abs(got - want).max()) <= FP64_ROUNDING


# ------------------------------------------------------------------------------------------------------------------ model vs reference
def test_model_agrees_with_the_golden(fx):
    for i, clip in enumerate(GI.clips_of(fx)):
        plain, mirrored = model(fx, clip), model(fx, clip, mirror=True)
        for k in GI.FIELDS:
            assert agrees(plain[k], fx[f"c{i}_{k}"]), (i, k)
        for k in GI.MIRROR_FIELDS:
            assert agrees(mirrored[k], fx[f"c{i}_mirror_{k}"]), (i, k)
        for k in ("pose_quat", "pose_aa", "trans_orig"):                     # the mirrored copy keeps the original's
            assert np.array_equal(mirrored[k], plain[k]), (i, k)


def test_model_agrees_with_the_reference_scripts(request, fx):
    """The statements of both scripts, executed (live) or as recorded."""
    with RefRecord(request) as R:
        for i, clip in enumerate(GI.clips_of(fx)):
            ref = GI.run_reference(clip, np.float64) if R.live else None
            plain, mirrored = model(fx, clip), model(fx, clip, mirror=True)
            for k in ("pose_quat_global", "pose_quat", "root_trans_offset"):
                assert agrees(plain[k], R.t(f"c{i}/{k}", lambda: ref[1][k]).numpy()), (i, k)
            for k in GI.MIRROR_FIELDS:
                assert agrees(mirrored[k], R.t(f"c{i}/mirror/{k}", lambda: ref[2][k]).numpy()), (i, k)
            dropped = R.obj(f"c{i}/dropped", lambda: ref[0] is None)
            assert dropped == (plain["pose_aa"].shape[0] < MI.MIN_FRAMES) == bool(fx[f"c{i}_dropped"])


@pytest.mark.skipif(not refload.available(), reason="reference checkout not present: the fixture stands in for it")
def test_generator_reproduces_the_fixture(fx):
    live = GI.generate(verbose=False)
    assert set(live) == set(fx)
    for k in sorted(fx):
        assert np.array_equal(live[k], fx[k]), k


# ------------------------------------------------------------------------------------------------------------------ the fixture's conditions
def test_no_sign_sits_within_fp32_rounding(fx):
    floor = float(fx["w_floor"])
    assert floor == 1e-3 and floor > 1000 * 4 * float(fx["err_pose_quat_global"])
    smallest = np.inf
    for clip in GI.clips_of(fx):
        res = model(fx, clip)
        decided = [res["global_products"][:, 1:, 3], res["local_products"][:, 1:, 3], res["global"][:, 1:, 3], res["pose_quat"][:, 1:, 3]]
        for w in decided:
            assert (np.abs(w) >= floor).all()
            smallest = min(smallest, float(np.abs(w).min()))
        for q in (res["global"][:, 1:], res["pose_quat"][:, 1:]):            # quat_pos made them so
            assert (q[..., 3] > 0).all()
    assert smallest >= float(fx["w_min"]) - 1e-12


def test_fixture_holds_the_cases(fx):
    clips = GI.clips_of(fx)
    assert sorted(c["framerate"] for c in clips) == [30.0, 30.0, 60.0, 100.0, 120.0]
    frames = [MI.decimate(len(c["poses"]), c["framerate"], c["bound"])[1] for c in clips]
    assert frames == [10, 11, 37, 2, 13] and sum(frames[:4]) % 8 != 0 and all(f <= 40 for f in frames)
    assert [bool(fx[f"c{i}_dropped"]) for i in range(5)] == [False, False, False, True, False]
    assert clips[3]["bound"] == 2 and clips[4]["bound"] == 13 and len(clips[4]["poses"]) > 13             # cut by bound: one dropped, one kept
    for c in clips:
        assert c["poses"].dtype == np.float32 and np.abs(c["poses"][[0, -1], 66:]).min() > 0                # non-zero hand columns going in
    aa = fx["c0_pose_aa"].reshape(10, 24, 3)
    assert (aa[:, 22:] == 0).all() and (aa[GI.ZERO_FRAME // 4] == 0).all()                                 # hands zeroed; a frame of exact zeros
    angle = np.linalg.norm(aa, axis=-1)
    for fr, joint, want in GI.SPECIAL:
        assert abs(angle[fr // 4, joint] - want) <= 1e-6 * want, (fr, joint)
    wanted = sorted(a for _, _, a in GI.SPECIAL)
    assert wanted[0] == 5e-4 and wanted[1] < 1e-3 < wanted[2] and wanted[1] > 0.999e-3 and wanted[2] < 1.001e-3
    assert sum(a > np.pi for a in wanted) >= 2 and max(wanted) > 2 * np.pi - 0.01
    for k in ("pose_aa", "trans_orig"):
        assert float(fx[f"err_{k}"]) == 0.0                                                                 # copies: exact in every precision
    for k in ("pose_quat_global", "pose_quat", "root_trans_offset"):
        assert 0 < float(fx[f"err_{k}"]) < 1e-6


def test_upright_false_is_the_model_alone(fx):
    """No statement of the reference runs without the upright factor: the branch is defined by the restatement, held here to its identities."""
    clip = GI.clips_of(fx)[1]
    res = model(fx, clip, upright_start=False)
    assert np.array_equal(res["pose_quat"], res["pose_local"]) and np.array_equal(res["pose_quat_global"], res["global"])
    up = model(fx, clip)
    back = MI.scipy_compose(up["pose_quat_global"], np.array([0.5, 0.5, 0.5, 0.5]))
    assert np.abs(back - MI.scipy_unit(res["global"])).max() <= FP64_ROUNDING


# ------------------------------------------------------------------------------------------------------------------ the entry point
def _args():
    """An argument struct the launcher would accept, over made-up device addresses (nothing here is launched: every test breaks one thing)."""
    keep = {"start": torch.tensor([0, 6], dtype=torch.int64), "skip": torch.tensor([2, 1], dtype=torch.int64),
            "frames": torch.tensor([3, 2], dtype=torch.int64), "par": (ctypes.c_int32 * 3)(-1, 0, 1)}
    a = _lib.MotionIngestArgs()
    for i, name in enumerate(("src_pose", "src_trans", "clip_src_start", "clip_skip", "clip_out_start", "out_rot", "out_trans")):
        setattr(a, name, 4096 * (i + 1))
    a.src_frames, a.num_clips, a.num_bodies, a.total_frames = 8, 2, 3, 5
    a.clip_src_start_host, a.clip_skip_host, a.clip_frames_host = keep["start"].data_ptr(), keep["skip"].data_ptr(), keep["frames"].data_ptr()
    a.parent_indices_host = ctypes.cast(keep["par"], ctypes.c_void_p)
    a.joint_map[:3], a.mirror_map[:3] = [0, 2, 3], [0, 2, 1]
    return a, keep


REFUSED = [("bodies_33", "num_bodies 33 not in [1,32]"), ("bodies_0", "num_bodies 0 not in [1,32]"), 
           ("negative", "negative clip / frame count"), ("null_pose", "null staging pointer"),
           ("null_trans", "null staging pointer"), ("empty", "staging buffers are empty"), ("null_clip_table", "null per-clip table"),
           ("null_host_table", "null host table"), ("null_parents", "null parent_indices_host"), ("null_out", "null output"),
           ("root_parent", "body 0 must be the root"), ("parent_order", "every parent must precede its child"), ("joint_map", "joint_map[1] = 24 is no SMPL joint"),
           ("mirror_map", "mirror_map[2] = 3 is no body"), ("no_frames", "clip 1 has 0 frames"), ("skip_0", "clip 0 has skip 0"),
           ("read_past", "clip 0 reads 3 staged frames from 0 in steps of 4, outside [0,8)"), ("read_before", "from -1 in steps of 1, outside [0,8)"),
           ("read_overflow", "clip 0 reads 4611686018427387904 staged frames"), ("frame_sum", "but total_frames is 6"),
           ("rot_align", "out_rot must be 16-byte aligned"), ("pose_quat_align", "out_pose_quat must be 16-byte aligned"), ("grid", "exceed the grid")]


@pytest.mark.parametrize("what,needle", REFUSED)
def test_refused_arguments(what, needle):
    a, keep = _args()
    if what == "bodies_33":
        a.num_bodies = 33
    elif what == "bodies_0":
        a.num_bodies = 0
    elif what == "negative":
        a.num_clips = -1
    elif what == "null_pose":
        a.src_pose = None
    elif what == "null_trans":
        a.src_trans = None
    elif what == "empty":
        a.src_frames = 0
    elif what == "null_clip_table":
        a.clip_skip = None
    elif what == "null_host_table":
        a.clip_frames_host = None
    elif what == "null_parents":
        a.parent_indices_host = None
    elif what == "null_out":
        a.out_trans = None
    elif what == "root_parent":
        keep["par"][0] = 0
    elif what == "parent_order":
        keep["par"][2] = 2
    elif what == "joint_map":
        a.joint_map[1] = 24
    elif what == "mirror_map":
        a.mirror_map[2] = 3
    elif what == "no_frames":
        keep["frames"][0], keep["frames"][1], keep["skip"][0] = 5, 0, 1
    elif what == "skip_0":
        keep["skip"][0] = 0
    elif what == "read_past":
        keep["skip"][0] = 4
    elif what == "read_overflow":                                   # (f - 1) * k would wrap around to a small number
        keep["frames"][0], keep["skip"][0] = 2 ** 62, 4
    elif what == "read_before":
        keep["start"][1] = -1
    elif what == "frame_sum":
        a.total_frames = 6
    elif what == "rot_align":
        a.out_rot = 4096 + 8
    elif what == "pose_quat_align":
        a.out_pose_quat = 8192 + 4
    elif what == "grid":
        keep["frames"][0], keep["frames"][1] = 2 ** 35, 1
        keep["skip"][0], keep["start"][1] = 1, 2 ** 35
        a.total_frames, a.src_frames = 2 ** 35 + 1, 2 ** 36
    lib = _lib.load()
    rc = lib.pulse_motion_ingest(ctypes.byref(a), None)
    msg = lib.pulse_last_error().decode()
    assert rc == INVALID and needle in msg and msg.startswith("pulse_motion_ingest: "), (what, rc, msg)


def test_entry_point_binding():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.MotionIngestArgs) == lib.pulse_sizeof_motion_ingest_args()
    assert lib.pulse_abi_version() == 36 == _lib.ABI_VERSION           # an added entry point: no existing struct or signature changed
    assert ctypes.sizeof(_lib.MotionBuildArgs) == lib.pulse_sizeof_motion_build_args()
    assert lib.pulse_motion_ingest(None, None) == INVALID and b"null args" in lib.pulse_last_error()
    assert lib.pulse_motion_ingest(ctypes.byref(_lib.MotionIngestArgs()), None) == 0          # no clips, no frames: nothing to do
    header = open(os.path.join(ROOT, "include", "pulse_hip.h")).read()
    assert "convert_amass_isaac.py:85-137" in header and "convert_amass_data.py:88-141" in header and "LABELLED 30 fps" in header
    assert header.index("2b'. Building") < header.index("2b'.1. Raw SMPL") < header.index("2b''. Evaluation")
    from pulse_amd.csrc import build
    assert ("motion_ingest.hip", build.NO_CONTRACT) in build.SOURCES


# ------------------------------------------------------------------------------------------------------------------ host logic, no device
def _raw(frames, rate=None, pose_key="poses", beta_key="betas", width=72):
    e = {pose_key: np.zeros((frames, width), dtype=np.float32), "trans": np.zeros((frames, 3)), beta_key: np.zeros(16), "gender": "male"}
    if rate is not None:
        e["mocap_framerate"] = np.array(rate)
    return e


def test_names_and_maps():
    assert sorted(syn.SMPL_BONE_ORDER_NAMES) == sorted(syn.SMPL_BODY_NAMES) and len(syn.SMPL_BONE_ORDER_NAMES) == 24
    jm = syn.smpl_joint_map()
    assert sorted(jm) == list(range(24)) and [syn.SMPL_BONE_ORDER_NAMES[s] for s in jm] == syn.SMPL_BODY_NAMES
    # SMPL's own tree (parents in joint order) is the humanoid's tree under the map
    smpl_parents = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]
    assert [-1 if p < 0 else jm[p] for p in syn.SMPL_PARENTS] == [smpl_parents[s] for s in jm]
    assert syn.mirror_body_map() == [0, 5, 6, 7, 8, 1, 2, 3, 4, 9, 10, 11, 12, 13, 19, 20, 21, 22, 23, 14, 15, 16, 17, 18]     # convert_amass_isaac.py:121


def test_plan_key_order_drops_and_mirror_keys():
    data = {"b": _raw(40, 30.0), "short": _raw(9, 30.0), "a": _raw(100, 120.0), "hz100": _raw(100, 100.0), "cut": _raw(60, 60.0), "gone": _raw(60, 60.0)}
    clips, dropped = ML.plan_smpl_clips(data, bounds={"cut": 12, "gone": 9})
    assert [c["key"] for c in clips] == ["b", "a", "hz100", "cut"] and dropped == ["short", "gone"]          # the data set's order
    assert [(c["skip"], c["frames"]) for c in clips] == [(1, 40), (4, 25), (3, 34), (2, 12)]                  # 100 Hz: skip 3, ceil(100 / 3)
    clips, _ = ML.plan_smpl_clips(data, bounds={"cut": 12, "gone": 9}, mirror=True)
    assert [c["key"] for c in clips] == ["b", "b_1", "a", "a_1", "hz100", "hz100_1", "cut", "cut_1"]
    assert [c["mirror"] for c in clips] == [False, True] * 4 and all(c["source"] == c["key"].removesuffix("_1") for c in clips)
    clips, _ = ML.plan_smpl_clips(data, mirror=True, im_eval=True)                                            # longest first, stable
    assert [c["key"] for c in clips] == ["b", "b_1", "hz100", "hz100_1", "cut", "cut_1", "gone", "gone_1", "a", "a_1"]
    clips, _ = ML.plan_smpl_clips(data, min_length=30)
    assert [c["key"] for c in clips] == ["b", "hz100", "cut", "gone"]
    with pytest.raises(ValueError, match="collides"):
        ML.plan_smpl_clips({"k": _raw(20), "k_1": _raw(20)}, mirror=True)


def test_plan_input_spellings_and_errors():
    both = {"x": _raw(20, None, "pose_aa", "beta"), "y": _raw(20, 60.0, "poses", "betas", width=156)}
    clips, dropped = ML.plan_smpl_clips(both)
    assert [(c["key"], c["skip"], c["frames"]) for c in clips] == [("x", 1, 20), ("y", 2, 10)] and not dropped   # no mocap_framerate: 30
    with pytest.raises(KeyError, match="pose_aa"):
        ML.plan_smpl_clips({"x": {"trans": np.zeros((20, 3)), "betas": np.zeros(10)}})
    with pytest.raises(KeyError, match="beta"):
        ML.plan_smpl_clips({"x": {"poses": np.zeros((20, 72)), "trans": np.zeros((20, 3))}})
    with pytest.raises(ValueError, match=r"\(F, >= 72\)"):
        ML.plan_smpl_clips({"x": _raw(20, width=66)})
    for bad in (25.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="clip 'x': mocap_framerate .* at least 30"):
            ML.plan_smpl_clips({"x": _raw(20, bad)})
    with pytest.raises(ValueError, match="negative"):
        ML.plan_smpl_clips({"x": _raw(20)}, bounds={"x": -2})
    with pytest.raises(ValueError, match="lives in HBM"):
        ML.MotionLib.from_smpl_data(both, (syn.SMPL_PARENTS, torch.zeros(1, 24, 3)), device="cpu")


def test_synthetic_smpl_data_is_raw_smpl():
    data, (parents, lt) = syn.synthetic_smpl_data(syn.make_generator(5), 3, framerate=[30, 60, 120], num_slots=2)
    assert parents == syn.SMPL_PARENTS and tuple(lt.shape) == (2, 24, 3)
    for (key, e), rate in zip(data.items(), (30, 60, 120)):
        f = e["poses"].shape[0]
        assert e["poses"].shape == (f, 72) and e["trans"].shape == (f, 3) and e["poses"].dtype == np.float32 and float(e["mocap_framerate"]) == rate
        assert 45 * (rate // 30) <= f <= 180 * (rate // 30) and np.abs(e["poses"][:, 66:]).max() > 0
    again, _ = syn.synthetic_smpl_data(syn.make_generator(5), 3, framerate=[30, 60, 120], num_slots=2)
    assert all(np.array_equal(data[k]["poses"], again[k]["poses"]) for k in data)
