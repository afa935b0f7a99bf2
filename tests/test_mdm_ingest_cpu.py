"""CPU: the yardsticks pulse_motion_euler_pose / pulse_motion_smooth are held to, and everything of the feature that needs no device.

  * tests/mdm_ingest_model.py (the fp64 restatement the GPU tests also use) agrees with tests/golden/mdm_ingest.npz -- the outputs of the
    reference's scripts/data_process/convert_data_mdm.py, tools/gen_golden_mdm_ingest.py -- to fp64 rounding, signs included (pose_quat to one
    fp32 ulp: poselib hands it back rounded to fp32, and the model rounds its own fp64 value);
  * the fixture's conditions (the tool's docstring) on the committed arrays;
  * quat_correct as defined (sequential) equals the prefix XOR of the raw tests, which is what the kernels compute, word for word;
  * kernels.gaussian_taps equals scipy's kernel bit for bit;
  * host planning and every refusal by name, the launchers' included (through the C ABI, over made-up addresses: nothing is launched).
"""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden_mdm_ingest as GM  # noqa: E402
import mdm_ingest_model as MM  # noqa: E402
from oracle import refload  # noqa: E402
from pulse_amd import _lib, kernels  # noqa: E402
from pulse_amd import synthetic as syn  # noqa: E402
from pulse_amd.env import motion_lib as ML  # noqa: E402

FP64_ROUNDING = 1e-13          # a few hundred fp64 operations on unit quaternions, angles up to pi and metre-sized translations
INVALID = -1


@pytest.fixture(scope="module")
def fx():
    return GM.load()


@pytest.fixture(scope="module")
def results(fx):
    return [GM.model(c) for c in GM.clips_of(fx)]


# ------------------------------------------------------------------------------------------------------------------ model vs reference
def test_model_agrees_with_the_golden(fx, results):
    for i, res in enumerate(results):
        for k in GM.FIELDS + ("euler_pose", "euler_trans"):
            got, want = res["trans_orig"] if k == "euler_trans" else res[k], fx[f"c{i}_{k}"]
            tol = 2.0 ** -23 if k == "pose_quat" else FP64_ROUNDING
            assert got.shape == want.shape and float(np.abs(got - want).max()) <= tol, (i, k, float(np.abs(got - want).max()))
            big = np.abs(want) > 1e-6
            assert np.array_equal(np.signbit(got[big]), np.signbit(want[big])), (i, k)
        assert (res["pose_aa"].reshape(-1, 24, 3)[:, 22:] == 0).all() and np.array_equal(res["pose_aa"][:, :66], res["euler_pose"][:, :66])
        assert abs(res["trans_orig"][0, 2] - 0.92) <= 1e-15                             # the first frame stands on the floor height


@pytest.mark.skipif(not refload.available(), reason="reference checkout not present: the fixture stands in for it")
def test_generator_reproduces_the_fixture(fx):
    pytest.importorskip("scipy")
    live = GM.generate(verbose=False)
    assert set(live) == set(fx)
    for k in sorted(fx):
        assert np.array_equal(live[k], fx[k]), k


# ------------------------------------------------------------------------------------------------------------------ the fixture's conditions
def test_fixture_meets_its_conditions(fx, results):
    assert [r["pose_aa"].shape[0] for r in results] == [10, 11, 26, 65] == list(GM.FRAMES)
    ok, figures = GM.conditions([GM.stage_of(r) for r in results])
    assert all(ok.values()), (ok, figures)
    # the margin (tools/gen_golden_mdm_ingest.py): what two fp32 evaluations of the norms of a step can differ by, from a kernel held to 4 x err
    # (e = 1e-6 per component, above this fixture's own err_pose_quat_global and tests/golden/motion_ingest.npz's)
    margin = 2.0 * (2.0 * (8.0 * 1e-6 + 2.0 ** -23) + 2.0 ** -21)
    assert float(fx["margin"]) == margin and float(fx["err_pose_quat_global"]) <= 1e-6
    assert figures["gap_min"] >= float(fx["gap_floor"]) == 1e-2 > 100 * margin
    assert abs(figures["gap_min"] - float(fx["gap_min"])) <= 1e-9 and figures["norm_min"] >= 0.5 and figures["w_min"] >= float(fx["w_floor"]) == 1e-3
    for k in GM.FIELDS + ("euler_pose", "euler_trans"):
        assert 0 < float(fx[f"err_{k}"]) < 1e-6, k
    # real sign changes, of the root and of a limb
    assert any(r["smooth"]["raw_flip"][:, 0].any() for r in results) and any(r["smooth"]["raw_flip"][:, 14:].any() for r in results)


def test_prefix_xor_is_quat_correct(results):
    """The definition runs frame by frame against the corrected predecessor; the kernels take the raw tests and scan them.  Equal whenever no
    step is a tie (the fixture's gap), because negating frame t - 1 swaps the two norms of the test at frame t."""
    for r in results:
        rot = r["ingest"]["pose_quat_global"]
        sm = r["smooth"]
        assert np.array_equal(MM.quat_correct(rot), sm["corrected"])
        for b in range(rot.shape[1]):
            assert np.array_equal(MM.quat_correct(rot[:, b]), sm["corrected"][:, b])
        bits, scanned = MM.sign_words(sm["raw_flip"])
        assert bits[0] == 0 and scanned[0] == 0                                        # frame 0 of a clip is never negated
        for b in range(rot.shape[1]):
            assert np.array_equal((scanned >> np.uint32(b)) & 1, sm["negated"][:, b].astype(np.uint32))
    # a 64-frame step of the scan hands a non-zero carry on
    assert MM.sign_words(results[3]["smooth"]["raw_flip"])[1][63] != 0


def test_filter_is_scipys(fx, results):
    ndimage = pytest.importorskip("scipy.ndimage")
    for r in results:
        sm = r["smooth"]
        for x, sigma, got in ((sm["corrected"], 2, sm["filtered"]), (r["ingest"]["root_trans_offset"], 3, sm["root_trans_offset"])):
            want = ndimage.gaussian_filter1d(x, sigma, axis=0, mode="nearest")
            assert got.shape == want.shape and float(np.abs(got - want).max()) <= 1e-15, sigma     # the same operations in the same order
    inner = MM.filter_nearest(results[3]["smooth"]["corrected"], 2.0, inner_first=True)
    assert float(np.abs(inner - results[3]["smooth"]["filtered"]).max()) <= 4 * 2.0 ** -53   # the other summation order: fp64 rounding apart


def test_gaussian_taps_are_scipys_bit_for_bit():
    filters = pytest.importorskip("scipy.ndimage._filters")
    for sigma, radius in ((2.0, 8), (3.0, 12), (2, None), (3, None), (0.5, None), (1.3, 5), (2.9, None), (0.1, None)):
        r = int(4.0 * float(sigma) + 0.5) if radius is None else radius
        want = filters._gaussian_kernel1d(float(sigma), 0, r)
        got = kernels.gaussian_taps(sigma, radius)
        assert len(got) == r + 1 and np.array_equal(np.array(got), want[r:]) and np.array_equal(want[:r + 1][::-1], want[r:])
        assert np.array_equal(MM.gaussian_kernel(float(sigma), r), want)
    assert kernels.gaussian_taps(2.0) == kernels.gaussian_weights(2.0, 8)               # motion_build's table


def test_gaussian_taps_refuse_by_name():
    with pytest.raises(ValueError, match=r"radius 13 \(sigma 3.2\) not in \[0,12\]"):
        kernels.gaussian_taps(3.2)
    with pytest.raises(ValueError, match=r"radius 13"):
        kernels.gaussian_taps(2.0, 13)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="not a positive finite number"):
            kernels.gaussian_taps(bad)


# ------------------------------------------------------------------------------------------------------------------ host logic, no device
def test_plan_mdm_clips(fx):
    clips = GM.clips_of(fx)
    result = {"thetas": [c["thetas"] if i % 2 else c["thetas"].reshape(-1, 72).astype(np.float64) for i, c in enumerate(clips)] + [np.zeros((9, 24, 3))],
              "root_translation": [c["root_translation"] for c in clips] + [np.zeros((9, 3))]}
    plan, dropped, thetas, roots = ML.plan_mdm_clips(result)
    assert dropped == ["4"] and [c["key"] for c in plan] == ["0", "1", "2", "3"] and [c["frames"] for c in plan] == [10, 11, 26, 65]
    assert all(c["skip"] == 1 and not c["mirror"] and c["source"] == c["key"] for c in plan)
    assert all(thetas[k].dtype == torch.float32 and tuple(thetas[k].shape) == (n, 72) and tuple(roots[k].shape) == (n, 3) for k, n in zip("0123", GM.FRAMES))
    assert np.array_equal(thetas["0"].numpy(), clips[0]["thetas"].reshape(-1, 72))
    plan, _, _, _ = ML.plan_mdm_clips(result, im_eval=True)
    assert [c["key"] for c in plan] == ["3", "2", "1", "0"]
    plan, _, _, _ = ML.plan_mdm_clips(result, min_length=26)
    assert [c["key"] for c in plan] == ["2", "3"]
    with pytest.raises(KeyError, match="thetas"):
        ML.plan_mdm_clips({"root_translation": []})
    with pytest.raises(ValueError, match="2 thetas sequences but 1 root_translation"):
        ML.plan_mdm_clips({"thetas": [np.zeros((10, 72))] * 2, "root_translation": [np.zeros((10, 3))]})
    with pytest.raises(ValueError, match=r"clip '0': thetas \(F, 24, 3\) or \(F, 72\)"):
        ML.plan_mdm_clips({"thetas": [np.zeros((10, 66))], "root_translation": [np.zeros((10, 3))]})


def test_smooth_argument_is_refused_by_name():
    S = ML.MotionLib._smooth_sigmas
    assert S(None, True, "x") is None and S(False, False, "x") is None and S(None, False, "x") is None
    assert S(True, True, "x") == (2.0, 3.0) and S({"sigma_rot": 1}, True, "x") == (1.0, 3.0) and S({"sigma_rot": 0, "sigma_trans": 0}, True, "x") == (0.0, 0.0)
    with pytest.raises(ValueError, match="from_smpl_data: smooth requires upright_start=True"):
        S(True, False, "from_smpl_data")
    with pytest.raises(ValueError, match=r"radius 13 \(sigma 3.2\) not in \[0,12\]"):
        S({"sigma_trans": 3.2}, True, "from_smpl_data")
    with pytest.raises(ValueError, match="sigma_rot / sigma_trans"):
        S({"sigma": 2}, True, "from_smpl_data")
    with pytest.raises(ValueError, match="MotionLib lives in HBM"):
        ML.MotionLib.from_mdm_data({"thetas": [], "root_translation": []}, None, device="cpu")
    with pytest.raises(ValueError, match="MotionLib lives in HBM"):
        ML.MotionLib.from_smpl_data({}, None, device="cpu", smooth=True)


def test_synthetic_mdm_result_turns_through_pi():
    """The seeded generator's clips really change sign: the root and the swung shoulder (body L_Shoulder and what hangs on it) are negated somewhere."""
    g = syn.make_generator(17)
    result, (parents, lt) = syn.synthetic_mdm_result(g, 3, frames=[40, 64, 30], num_slots=5)
    again, _ = syn.synthetic_mdm_result(syn.make_generator(17), 3, frames=[40, 64, 30], num_slots=5)
    assert parents == list(syn.SMPL_PARENTS) and tuple(lt.shape) == (5, 24, 3)
    shoulder = syn.SMPL_BODY_NAMES.index("L_Shoulder")
    for i, n in enumerate((40, 64, 30)):
        th, tr = result["thetas"][i], result["root_translation"][i]
        assert th.shape == (n, 24, 3) and th.dtype == np.float32 and tr.shape == (n, 3) and np.array_equal(th, again["thetas"][i])
        res = MM.mdm_clip(th, tr, syn.SMPL_PARENTS, syn.smpl_joint_map())
        raw, gap = res["smooth"]["raw_flip"], res["smooth"]["gap"]
        assert raw[:, 0].any() and raw[:, shoulder].any(), i
        assert gap.min() > 1e-2                                                         # no step near a tie
        # the local rotation of the shoulder joint itself passes a rotation angle of pi between two frames
        aa = res["euler_pose"].reshape(n, 24, 3)[:, syn.SMPL_BONE_ORDER_NAMES.index("L_Shoulder")]
        q = MM.MI.from_rotvec(aa)
        assert ((q[:-1] * q[1:]).sum(-1) < 0).any() and np.linalg.norm(aa, axis=-1).max() > 3.0


# ------------------------------------------------------------------------------------------------------------------ the entry points
def _smooth_args():
    """An argument struct pulse_motion_smooth would accept, over made-up device addresses (nothing here is launched: every test breaks one thing)."""
    keep = {"frames": torch.tensor([3, 2], dtype=torch.int64), "par": (ctypes.c_int32 * 3)(-1, 0, 1)}
    a = _lib.MotionSmoothArgs()
    for i, name in enumerate(("in_rot", "in_trans", "clip_start", "sign_words", "out_rot", "out_trans", "out_pose_quat")):
        setattr(a, name, 1 << 20 << i)
    a.total_frames, a.num_clips, a.num_bodies, a.radius_rot, a.radius_trans = 5, 2, 3, 8, 12
    a.clip_frames_host, a.parent_indices_host = keep["frames"].data_ptr(), ctypes.cast(keep["par"], ctypes.c_void_p)
    return a, keep


def _euler_args():
    keep = {"frames": torch.tensor([3, 2], dtype=torch.int64)}
    a = _lib.MotionEulerPoseArgs()
    for i, name in enumerate(("src_theta", "src_trans", "clip_start", "out_pose", "out_trans")):
        setattr(a, name, 1 << 20 << i)
    a.total_frames, a.num_clips, a.clip_frames_host = 5, 2, keep["frames"].data_ptr()
    return a, keep


SMOOTH_REFUSED = [("bodies_33", "num_bodies 33 not in [1,32]"), ("bodies_0", "num_bodies 0 not in [1,32]"), ("negative", "negative clip / frame count"),
                  ("null_in", "null input pointer (in_rot / in_trans)"), ("null_trans", "null input pointer (in_rot / in_trans)"),
                  ("null_clip_table", "null clip table"), ("null_host_table", "null clip table"), ("null_words", "null workspace (sign_words)"),
                  ("null_out", "null output (out_rot / out_trans)"), ("null_parents", "null parent_indices_host"),
                  ("root_parent", "body 0 must be the root"), ("parent_order", "every parent must precede its child"),
                  ("radius_rot", "radius_rot 13 not in [-1,12]"), ("radius_trans", "radius_trans -2 not in [-1,12]"),
                  ("no_frames", "clip 1 has 0 frames"), ("frame_sum", "the clips hold 5 frames but total_frames is 6"),
                  ("frame_overflow", "the clips hold more frames than total_frames 5 (at clip 0)"),
                  ("in_align", "in_rot must be 16-byte aligned"), ("rot_align", "out_rot must be 16-byte aligned"),
                  ("pose_quat_align", "out_pose_quat must be 16-byte aligned"), ("alias_rot", "out_rot overlaps in_rot"),
                  ("alias_rot_tail", "out_rot overlaps in_rot"), ("alias_pose_quat", "out_pose_quat overlaps in_rot"),
                  ("alias_outputs", "out_pose_quat overlaps out_rot"), ("alias_trans", "out_trans overlaps in_trans"), ("alias_words", "sign_words overlaps a data buffer"),
                  ("grid", "exceed the grid")]


@pytest.mark.parametrize("what,needle", SMOOTH_REFUSED)
def test_smooth_refuses(what, needle):
    a, keep = _smooth_args()
    if what == "bodies_33":
        a.num_bodies = 33
    elif what == "bodies_0":
        a.num_bodies = 0
    elif what == "negative":
        a.total_frames = -1
    elif what == "null_in":
        a.in_rot = None
    elif what == "null_trans":
        a.in_trans = None
    elif what == "null_clip_table":
        a.clip_start = None
    elif what == "null_host_table":
        a.clip_frames_host = None
    elif what == "null_words":
        a.sign_words = None
    elif what == "null_out":
        a.out_rot = None
    elif what == "null_parents":
        a.parent_indices_host = None
    elif what == "root_parent":
        keep["par"][0] = 0
    elif what == "parent_order":
        keep["par"][2] = 2
    elif what == "radius_rot":
        a.radius_rot = 13
    elif what == "radius_trans":
        a.radius_trans = -2
    elif what == "no_frames":
        keep["frames"][0], keep["frames"][1] = 5, 0
    elif what == "frame_sum":
        a.total_frames = 6
    elif what == "frame_overflow":
        keep["frames"][0] = 2 ** 63 - 1
    elif what == "in_align":
        a.in_rot = (1 << 20) + 4
    elif what == "rot_align":
        a.out_rot = (1 << 24) + 8
    elif what == "pose_quat_align":
        a.out_pose_quat = (1 << 26) + 4
    elif what == "alias_rot":
        a.out_rot = a.in_rot
    elif what == "alias_rot_tail":
        a.out_rot = a.in_rot + 5 * 3 * 16 - 16                     # the last quaternion of the input
    elif what == "alias_pose_quat":
        a.out_pose_quat = a.in_rot + 16
    elif what == "alias_outputs":
        a.out_pose_quat = a.out_rot
    elif what == "alias_trans":
        a.out_trans = a.in_trans + 8
    elif what == "alias_words":
        a.sign_words = a.out_rot + 5 * 3 * 16 - 4                  # the last float of out_rot
    elif what == "grid":
        keep["frames"][0], keep["frames"][1] = 2 ** 35, 1
        a.total_frames = 2 ** 35 + 1
        for i, name in enumerate(("in_rot", "out_rot", "out_pose_quat", "in_trans", "out_trans")):       # far enough apart not to overlap
            setattr(a, name, (i + 1) << 44)
    lib = _lib.load()
    rc = lib.pulse_motion_smooth(ctypes.byref(a), None)
    msg = lib.pulse_last_error().decode()
    assert rc == INVALID and needle in msg and msg.startswith("pulse_motion_smooth: "), (what, rc, msg)


EULER_REFUSED = [("negative", "negative clip / frame count"), ("null_theta", "null input pointer (src_theta / src_trans)"),
                 ("null_clip_table", "null clip table"), ("null_host_table", "null clip table"), ("null_out", "null output (out_pose / out_trans)"),
                 ("no_frames", "clip 0 has 0 frames"), ("frame_sum", "the clips hold 5 frames but total_frames is 6"),
                 ("alias_pose", "out_pose overlaps src_theta"), ("alias_trans", "out_trans overlaps src_trans"), ("grid", "exceed the grid")]


@pytest.mark.parametrize("what,needle", EULER_REFUSED)
def test_euler_pose_refuses(what, needle):
    a, keep = _euler_args()
    if what == "negative":
        a.num_clips = -2
    elif what == "null_theta":
        a.src_theta = None
    elif what == "null_clip_table":
        a.clip_start = None
    elif what == "null_host_table":
        a.clip_frames_host = None
    elif what == "null_out":
        a.out_trans = None
    elif what == "no_frames":
        keep["frames"][0], keep["frames"][1] = 0, 5
    elif what == "frame_sum":
        a.total_frames = 6
    elif what == "alias_pose":
        a.out_pose = a.src_theta + 4 * 288
    elif what == "alias_trans":
        a.out_trans = a.src_trans
    elif what == "grid":
        keep["frames"][0], keep["frames"][1] = 2 ** 35, 1
        a.total_frames = 2 ** 35 + 1
        for i, name in enumerate(("src_theta", "out_pose", "src_trans", "out_trans")):
            setattr(a, name, (i + 1) << 46)
    lib = _lib.load()
    rc = lib.pulse_motion_euler_pose(ctypes.byref(a), None)
    msg = lib.pulse_last_error().decode()
    assert rc == INVALID and needle in msg and msg.startswith("pulse_motion_euler_pose: "), (what, rc, msg)


def test_entry_point_binding():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.MotionSmoothArgs) == lib.pulse_sizeof_motion_smooth_args()
    assert ctypes.sizeof(_lib.MotionEulerPoseArgs) == lib.pulse_sizeof_motion_euler_pose_args()
    assert lib.pulse_abi_version() == 36 == _lib.ABI_VERSION           # added entry points: no existing struct or signature changed
    assert ctypes.sizeof(_lib.MotionIngestArgs) == lib.pulse_sizeof_motion_ingest_args()
    for entry, struct in ((lib.pulse_motion_smooth, _lib.MotionSmoothArgs), (lib.pulse_motion_euler_pose, _lib.MotionEulerPoseArgs)):
        assert entry(None, None) == INVALID and b"null args" in lib.pulse_last_error()
        assert entry(ctypes.byref(struct()), None) == 0                # no clips, no frames: nothing to do
    header = open(os.path.join(ROOT, "include", "pulse_hip.h")).read()
    assert "convert_data_mdm.py" in header and ":48-61" in header and ":128-141" in header
    assert header.index("2b'.1. Raw SMPL") < header.index("2b'.1a. Generated") < header.index("2b'.2. A recorded rollout")
    assert kernels.SMOOTH_MAX_RADIUS == 12 and "#define PULSE_SMOOTH_MAX_RADIUS 12" in header
    from pulse_amd.csrc import build
    assert ("motion_smooth.hip", build.NO_CONTRACT) in build.SOURCES


def test_wrappers_refuse_before_the_library(fx):
    """kernels.motion_smooth / motion_euler_pose on CPU tensors: a TypeError that names the tensor, nothing reaches the library."""
    rot, trans = torch.zeros(5, 3, 4), torch.zeros(5, 3)
    with pytest.raises(TypeError, match="in_rot: expected a CUDA tensor"):
        kernels.motion_smooth(rot.clone(), trans.clone(), in_rot=rot, in_trans=trans, clip_frames=torch.tensor([3, 2]), parents=[-1, 0, 1])
    with pytest.raises(TypeError, match="src_theta: expected a CUDA tensor"):
        kernels.motion_euler_pose(torch.zeros(5, 72), trans.clone(), src_theta=torch.zeros(5, 72), src_trans=trans, clip_frames=torch.tensor([3, 2]))
    assert np.abs(np.array(kernels.quat_matrix(kernels.MDM_ROOT_QUAT)) - MM.quat_matrix(MM.ROOT_QUAT).ravel()).max() <= 1e-15
    assert np.abs(np.array(kernels.MDM_ROOT_QUAT) - MM.ROOT_QUAT).max() <= 1e-15
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert ML.plan_mdm_clips({"thetas": [fx["c0_thetas"]], "root_translation": [fx["c0_root_translation"]]})[1] == []
