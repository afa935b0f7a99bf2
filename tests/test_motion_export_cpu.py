"""CPU: the yardsticks pulse_motion_export is held to, and everything of the feature that needs no device.

  * tests/motion_export_model.py (the fp64 numpy restatement the GPU tests also use) agrees with tests/golden/motion_export.npz -- the outputs of
    the reference's own statements, tools/gen_golden_motion_export.py -- to fp64 rounding, signs included; the model's segmentation and its
    ``states`` fields are checked against the body of Humanoid._write_states_to_file run live where the reference checkout is present
    (RefRecord), and replayed from tests/golden/ref/ elsewhere;
  * on the committed arrays, every quaternion whose sign the reference decides has |w| >= the fixture's floor, 1e-3; nothing is masked;
  * the fixture's cases are the ones the generator describes, and a fresh run reproduces it where the reference is present;
  * ``segment_recording``'s rule against its restatement on the edge recordings;
  * the entry point's struct as the C compiler lays it out, the ABI version, and every message of the launcher's argument checks;
  * ``export_motion`` raises by name for a 52-body skeleton; the recorder's record / clear / capacity on a stand-in task."""
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

import gen_golden_motion_export as GX  # noqa: E402
import motion_export_model as MX  # noqa: E402
import motion_ingest_model as MI  # noqa: E402
from oracle import refload  # noqa: E402
from oracle.refrecord import RefRecord  # noqa: E402
from pulse_amd import _lib  # noqa: E402
from pulse_amd import synthetic as syn  # noqa: E402
from pulse_amd.env import motion_export as ME  # noqa: E402

FP64_ROUNDING = 1e-14          # a few dozen fp64 operations on unit quaternions, rotation vectors below pi and metre-sized translations
INVALID = -1
EDGE_RECORDINGS = MX.EDGE_RECORDINGS


@pytest.fixture(scope="module")
def fx():
    return GX.load()


@pytest.fixture(scope="module")
def res(fx):
    frames, dofs = MX.gather(fx["rb"], fx["dof_pos"], GX.segs_of(fx))
    return MX.export_frames(frames, dofs, syn.SMPL_PARENTS, syn.smpl_joint_map(), root_offset=fx["root_offset"])


def agrees(got, want):
    got = np.asarray(got).reshape(want.shape)
    return np.array_equal(np.signbit(got), np.signbit(want)) and float(np.abs(got - want).max()) <= FP64_ROUNDING


# ------------------------------------------------------------------------------------------------------------------ model vs reference
def test_model_agrees_with_the_golden(fx, res):
    for k in GX.FIELDS:
        assert agrees(res[k], fx[k]), k
    for k, field in (("body_quat", "states_body_quat"), ("dof_pos", "states_dof_pos"), ("root_trans_offset", "states_trans")):
        assert agrees(res[k], fx[field]), field
    frames, _ = MX.gather(fx["rb"], None, GX.segs_of(fx))
    assert np.array_equal(frames[:, 0].astype(np.float64), fx["states_root_states_seg"])


def test_model_round_trip_agrees_with_the_golden(fx, res):
    """export -> ingest: the model's pose_aa / trans_orig through the ingest model is the reference's own round trip."""
    sel = fx["roundtrip_frames"]
    back = MI.ingest_clip(res["pose_aa"][sel], res["trans_orig"][sel], 30.0, syn.SMPL_PARENTS, syn.smpl_joint_map(), root_offset=fx["root_offset"])
    assert agrees(back["pose_quat_global"], fx["roundtrip_pose_quat_global"]) and agrees(back["root_trans_offset"], fx["roundtrip_root_trans_offset"])
    # and the round trip is the identity up to the sign the upright factor leaves and the fp32 rounding poselib puts into pose_quat
    rot = MI.scipy_unit(res["pose_quat_global"][sel])
    dot = np.abs((rot * fx["roundtrip_pose_quat_global"]).sum(-1))
    assert float((1.0 - dot).max()) < 1e-12 and float(np.abs(back["root_trans_offset"] - res["root_trans_offset"][sel]).max()) < 1e-7
    assert float(fx["err_roundtrip_pose_quat_global"]) > 0 and float(fx["err_roundtrip_root_trans_offset"]) == 0.0


def test_segmentation_and_states_against_the_reference_method(request, fx, res):
    """The body of _write_states_to_file, executed (live) or as recorded: keys, segment lengths and every field of the dump."""
    segs = MX.segments(fx["progress"])
    keys = MX.segment_keys(segs)
    with RefRecord(request) as R:
        ref = GX.run_write_states(fx["rb"], fx["dof_pos"], fx["progress"], np.float64) if R.live else None
        assert R.obj("keys", lambda: list(ref)) == keys
        assert R.obj("frames", lambda: [int(ref[k]["trans"].shape[0]) for k in ref]) == [s[2] for s in segs]
        assert R.obj("fps", lambda: sorted({int(ref[k]["fps"]) for k in ref})) == [60]                       # the literal, whatever the control rate
        assert R.obj("betas_row", lambda: [int(ref[k]["betas"][0]) // 17 for k in ref]) == [s[0] for s in segs]   # humanoid_shapes[env]
        at = 0
        for k, (e, t0, n) in zip(keys, segs):
            for mine, field in (("body_quat", "body_quat"), ("dof_pos", "dof_pos"), ("root_trans_offset", "trans")):
                assert agrees(res[mine][at:at + n], R.t(f"{k}/{field}", lambda: ref[k][field]).numpy()), (k, field)
            assert np.array_equal(R.t(f"{k}/root_states_seg", lambda: ref[k]["root_states_seg"]).numpy(), fx["rb"][t0:t0 + n, e, 0].astype(np.float64))
            at += n
    for rec in EDGE_RECORDINGS:                               # every env's segments partition [0, T)
        prog = np.asarray(rec)
        by_env = {}
        for e, t0, n in MX.segments(prog):
            assert n >= 1 and t0 == by_env.get(e, 0)
            by_env[e] = t0 + n
        assert by_env == {e: prog.shape[0] for e in range(prog.shape[1])}


@pytest.mark.skipif(not refload.available(), reason="reference checkout not present: the fixture stands in for it")
def test_generator_reproduces_the_fixture(fx):
    live = GX.generate(verbose=False)
    assert set(live) == set(fx)
    for k in sorted(fx):
        assert np.array_equal(live[k], fx[k]), k


# ------------------------------------------------------------------------------------------------------------------ the fixture's conditions
def test_no_sign_sits_within_fp32_rounding(fx, res):
    floor = float(fx["w_floor"])
    assert floor == 1e-3 and floor > 1000 * 4 * float(fx["err_pose_quat"])
    w = MX.decided_w(res)
    assert (w >= floor).all() and float(w.min()) >= float(fx["w_min"]) - 1e-12
    assert (res["pose_quat"][:, 1:, 3] > 0).all()                                       # quat_pos made them so


def test_fixture_holds_the_cases(fx, res):
    rb, progress = fx["rb"], fx["progress"]
    assert rb.shape == (7, 9, 24, 13) and rb.dtype == np.float32 and fx["dof_pos"].shape == (7, 9, 69) and progress.shape == (7, 9)
    segs = GX.segs_of(fx)
    assert segs == MX.segments(progress) and [s[2] for s in segs] == GX.SEGMENT_FRAMES and sum(GX.SEGMENT_FRAMES) == 63 and 63 % 8 != 0
    per_env = {e: [s[2] for s in segs if s[0] == e] for e in range(9)}
    assert per_env[0] == [7]                                                            # never resets
    assert 1 in per_env[1] and per_env[8] == [1] * 7                                    # 1-frame segments
    assert per_env[2] == [7] and (np.abs(np.diff(progress[:, 2])) == 1).all() and (np.diff(progress[:, 2]) < 0).any()   # a reset by exactly 1: no split
    assert per_env[3] == [6, 1]                                                         # a split at the last step
    starts = np.cumsum([0] + GX.SEGMENT_FRAMES[:-1])
    assert (starts % 8 != 0)[1:].sum() >= 15                                            # segment boundaries off the workgroup grid
    at = {(t, e): i for i, (t, e) in enumerate((t0 + k, e) for e, t0, n in segs for k in range(n))}
    aa = fx["pose_aa"].reshape(63, 24, 3)
    angle = np.linalg.norm(aa, axis=-1)
    jm = syn.smpl_joint_map()
    for t, e, s, want in GX.SPECIAL:
        i = at[(t, e)]
        if want is None:
            assert (aa[i, s] == 0).all() and np.array_equal(fx["pose_quat"][i, jm.index(s)], [0, 0, 0, 1])      # exact identity
        else:
            lo, hi = GX.ANGLE_WINDOW[want]
            assert lo < angle[i, s] < hi, (t, e, s, angle[i, s])
    lo, hi = GX.ANGLE_WINDOW[0.9999e-3][1], GX.ANGLE_WINDOW[1.0001e-3][0]
    assert lo < 1e-3 < hi                                                               # the two sit on either side of as_rotvec's series boundary
    for t, e, b in GX.NEGATED:
        assert rb[t, e, b, 6] < 0                                                       # stored as -q
    assert fx["pose_quat"][at[(4, 0)], 0, 3] < 0 and res["local_products"][at[(4, 0)], 7, 3] < 0    # a root as_rotvec flips, a product quat_pos flips
    for t, e, b, norm in GX.SCALED:
        assert abs(np.linalg.norm(rb[t, e, b, 3:7].astype(np.float64)) - norm) < 2e-7
    assert (aa[:42, 22:] == 0).all() and np.abs(aa[42:, 22:]).min() > 0                 # hands: identity on the round-trip frames only
    assert fx["roundtrip_frames"].tolist() == list(range(42))
    dof = fx["dof_pos"].reshape(7, 9, 23, 3)
    for t, e, j, mag in GX.DOF_SPECIAL:
        assert abs(np.linalg.norm(dof[t, e, j].astype(np.float64)) - mag) <= 1e-6 * max(mag, 1e-3)
    for k in ("pose_quat_global", "root_trans_offset", "states_trans", "states_root_states_seg", "states_dof_pos"):
        assert float(fx[f"err_{k}"]) == 0.0                                             # copies: exact in every precision
    for k in ("pose_quat", "pose_aa", "trans_orig", "states_body_quat", "roundtrip_pose_quat_global"):
        assert 0 < float(fx[f"err_{k}"]) < 1e-6


def test_model_functions_against_torch_utils(request):
    """quat_to_exp_map / exp_map_to_quat of the model against the reference's torch functions (the non-upright branch and the dump rest on them)."""
    g = np.random.default_rng(5)
    q = g.standard_normal((64, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    q[0] = [0, 0, 0, 1]
    e = g.standard_normal((64, 3)) * g.random((64, 1)) * 3.5
    e[0], e[1] = 0.0, [4e-6, 0, 0]
    with RefRecord(request) as R:
        tu = refload.torch_utils() if R.live else None
        want_e = R.t("quat_to_exp_map", lambda: tu.quat_to_exp_map(torch.from_numpy(q))).numpy()
        want_q = R.t("exp_map_to_quat", lambda: tu.exp_map_to_quat(torch.from_numpy(e))).numpy()
    assert float(np.abs(MX.quat_to_exp_map(q) - want_e).max()) <= 1e-12 and float(np.abs(MX.exp_map_to_quat(e) - want_q).max()) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ segment_recording
def test_segment_recording_rule(fx):
    for rec in [fx["progress"]] + [np.asarray(r) for r in EDGE_RECORDINGS]:
        got = ME.segment_recording(torch.as_tensor(rec, dtype=torch.int64))
        want = MX.segments(rec)
        assert list(zip(got["env"].tolist(), got["t0"].tolist(), got["frames"].tolist())) == want
        assert got["keys"] == MX.segment_keys(want)
        assert int(got["frames"].sum()) == rec.size
    got = ME.segment_recording(torch.tensor([[0, 5], [1, 6], [0, 0], [1, 1]]))
    assert got["keys"] == ["0_0", "1_0", "1_1"] and got["frames"].tolist() == [4, 2, 2]        # the quirk: env 0's reset moved progress by 1
    with pytest.raises(TypeError, match="int64"):
        ME.segment_recording(torch.zeros(3, 2))


# ------------------------------------------------------------------------------------------------------------------ the entry point
def _args():
    """An argument struct the launcher would accept, over made-up device addresses (nothing here is launched: every test breaks one thing)."""
    keep = {"env": torch.tensor([0, 1], dtype=torch.int64), "t0": torch.tensor([0, 2], dtype=torch.int64),
            "frames": torch.tensor([3, 2], dtype=torch.int64), "par": (ctypes.c_int32 * 3)(-1, 0, 1)}
    a = _lib.MotionExportArgs()
    for i, name in enumerate(("rb", "dof_pos", "seg_env", "seg_t0", "seg_out_start", "out_rot", "out_trans")):
        setattr(a, name, 4096 * (i + 1))
    a.rb_stride_t, a.rb_stride_n, a.rb_stride_b, a.dof_stride_t, a.dof_stride_n = 2 * 3 * 13, 3 * 13, 13, 2 * 6, 6
    a.num_steps, a.num_envs, a.num_bodies, a.num_segments, a.total_frames, a.upright_start = 4, 2, 3, 2, 5, 1
    a.seg_env_host, a.seg_t0_host, a.seg_frames_host = keep["env"].data_ptr(), keep["t0"].data_ptr(), keep["frames"].data_ptr()
    a.parent_indices_host = ctypes.cast(keep["par"], ctypes.c_void_p)
    a.joint_map[:3] = [0, 2, 1]
    return a, keep


REFUSED = [("bodies_33", "num_bodies 33 not in [1,32]"), ("bodies_0", "num_bodies 0 not in [1,32]"), ("negative", "negative segment / frame count"),
           ("null_rb", "null recording (rb)"), ("empty", "the recording is empty"), ("body_stride", "at least 13 floats between bodies"),
           ("dof_stride", "negative dof_pos stride"), ("null_seg_table", "null per-segment table"), ("null_host_table", "null host table"),
           ("null_parents", "null parent_indices_host"), ("null_out", "null output (out_rot / out_trans)"),
           ("body_quat_no_dof", "out_body_quat / out_dof_pos need dof_pos"), ("dof_out_no_dof", "out_body_quat / out_dof_pos need dof_pos"),
           ("pose_no_dof", "without upright_start out_pose_quat / out_pose_aa need dof_pos"),
           ("root_parent", "body 0 must be the root"), ("parent_order", "every parent must precede its child"),
           ("joint_map_range", "joint_map[1] = 3 is no SMPL joint"), ("joint_map_twice", "joint_map[2] = 0 is taken twice"),
           ("no_frames", "segment 1 has 0 frames"), ("env_past", "segment 1 is of env 2, outside [0,2)"), ("env_before", "segment 0 is of env -1"),
           ("read_past", "segment 1 reads 2 steps from 3, outside [0,4)"), ("read_before", "segment 0 reads 3 steps from -1"),
           ("read_overflow", "segment 0 reads 9223372036854775807 steps"), ("frame_sum", "but total_frames is 6"),
           ("rot_align", "out_rot must be 16-byte aligned"), ("pose_quat_align", "out_pose_quat must be 16-byte aligned"),
           ("body_quat_align", "out_body_quat must be 16-byte aligned")]


@pytest.mark.parametrize("what,needle", REFUSED)
def test_refused_arguments(what, needle):
    a, keep = _args()
    if what == "bodies_33":
        a.num_bodies = 33
    elif what == "bodies_0":
        a.num_bodies = 0
    elif what == "negative":
        a.num_segments = -1
    elif what == "null_rb":
        a.rb = None
    elif what == "empty":
        a.num_steps = 0
    elif what == "body_stride":
        a.rb_stride_b = 12
    elif what == "dof_stride":
        a.dof_stride_n = -6
    elif what == "null_seg_table":
        a.seg_t0 = None
    elif what == "null_host_table":
        a.seg_frames_host = None
    elif what == "null_parents":
        a.parent_indices_host = None
    elif what == "null_out":
        a.out_trans = None
    elif what == "body_quat_no_dof":
        a.dof_pos, a.out_body_quat = None, 65536
    elif what == "dof_out_no_dof":
        a.dof_pos, a.out_dof_pos = None, 65536
    elif what == "pose_no_dof":
        a.dof_pos, a.upright_start, a.out_pose_aa = None, 0, 65536
    elif what == "root_parent":
        keep["par"][0] = 0
    elif what == "parent_order":
        keep["par"][2] = 2
    elif what == "joint_map_range":
        a.joint_map[1] = 3
    elif what == "joint_map_twice":
        a.joint_map[2] = 0
    elif what == "no_frames":
        keep["frames"][0], keep["frames"][1] = 4, 0
    elif what == "env_past":
        keep["env"][1] = 2
    elif what == "env_before":
        keep["env"][0] = -1
    elif what == "read_past":
        keep["t0"][1] = 3
    elif what == "read_before":
        keep["t0"][0] = -1
    elif what == "read_overflow":                                   # t0 + frames would wrap around
        keep["frames"][0], keep["t0"][0] = 2 ** 63 - 1, 1
    elif what == "frame_sum":
        a.total_frames = 6
    elif what == "rot_align":
        a.out_rot = 4096 + 8
    elif what == "pose_quat_align":
        a.out_pose_quat = 8192 + 4
    elif what == "body_quat_align":
        a.out_body_quat = 8192 + 12
    lib = _lib.load()
    rc = lib.pulse_motion_export(ctypes.byref(a), None)
    msg = lib.pulse_last_error().decode()
    assert rc == INVALID and needle in msg and msg.startswith("pulse_motion_export: "), (what, rc, msg)


def test_entry_point_binding():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.MotionExportArgs) == lib.pulse_sizeof_motion_export_args()
    assert lib.pulse_abi_version() == 36 == _lib.ABI_VERSION           # an added entry point: no existing struct or signature changed
    assert ctypes.sizeof(_lib.MotionIngestArgs) == lib.pulse_sizeof_motion_ingest_args()
    assert lib.pulse_motion_export(None, None) == INVALID and b"null args" in lib.pulse_last_error()
    assert lib.pulse_motion_export(ctypes.byref(_lib.MotionExportArgs()), None) == 0          # zero segments: nothing to do
    from pulse_amd.csrc import build
    assert ("motion_export.hip", build.NO_CONTRACT) in build.SOURCES


# ------------------------------------------------------------------------------------------------------------------ host logic, no device
def test_export_motion_refuses_by_name():
    parents = syn.skeleton("smplx")["parents"]
    rb = torch.zeros(2, 1, 52, 13)
    with pytest.raises(NotImplementedError, match="52 bodies: only the 24-body SMPL humanoid"):
        ME.export_motion(rb, torch.zeros(2, 1, dtype=torch.int64), (parents, torch.zeros(1, 52, 3)), fps=30)
    trees = (syn.SMPL_PARENTS, torch.zeros(1, 24, 3))
    with pytest.raises(ValueError, match="form 'tables'"):
        ME.export_motion(torch.zeros(2, 1, 24, 13), torch.zeros(2, 1, dtype=torch.int64), trees, fps=30, form="tables")
    with pytest.raises(TypeError, match="CUDA tensor"):
        ME.export_motion(torch.zeros(2, 1, 24, 13), torch.zeros(2, 1, dtype=torch.int64), trees, fps=30)


def test_recorder_surface():
    """record / clear / capacity on the attributes both task families carry (sim.rigid_body_state, sim.dof_pos, progress_buf); copies, not views."""
    import types
    sim = types.SimpleNamespace(rigid_body_state=torch.zeros(2, 24, 13), dof_pos=torch.zeros(2, 69))
    task = types.SimpleNamespace(sim=sim, progress_buf=torch.zeros(2, dtype=torch.int64), dt=1 / 30, _has_upright_start=True, humanoid_type="smpl")
    rec = ME.MotionRecorder(task, 3)
    for t in range(3):
        sim.rigid_body_state += 1
        sim.dof_pos -= 1
        task.progress_buf += 1
        rec.record()
    assert rec.steps == 3 and rec.rb.shape == (3, 2, 24, 13) and rec.rb[:, 0, 0, 0].tolist() == [1, 2, 3] and rec.dof_pos[:, 1, 5].tolist() == [-1, -2, -3]
    assert rec.progress.dtype == torch.int64 and rec.progress[:, 0].tolist() == [1, 2, 3]
    with pytest.raises(RuntimeError, match="3 steps of capacity"):
        rec.record()
    parents, lt = rec.skeleton_trees()
    assert parents == syn.SMPL_PARENTS and tuple(lt.shape) == (1, 24, 3)
    rec.clear()
    assert rec.steps == 0
    with pytest.raises(ValueError, match="nothing recorded"):
        rec.export()
    with pytest.raises(ValueError, match="capacity 0"):
        ME.MotionRecorder(task, 0)


def test_export_pickles_as_a_plain_dict():
    """joblib.dump(export, path) is the caller's last line: what is written must load where this package is not installed."""
    import pickle
    out = ME.MotionExport({"0_0": {"pose_aa": np.zeros((2, 72), dtype=np.float32), "fps": 30}})
    out.dropped, out.segments = [("0_1", 1)], {"keys": ["0_0"], "env": torch.tensor([0]), "t0": torch.tensor([0]), "frames": torch.tensor([2])}
    data = pickle.dumps(out)
    assert b"pulse_amd" not in data and b"torch" not in data
    back = pickle.loads(data)
    assert type(back) is dict and list(back) == ["0_0"] and back["0_0"]["fps"] == 30 and np.array_equal(back["0_0"]["pose_aa"], out["0_0"]["pose_aa"])
    assert out.dropped_frames == 1
