"""CPU: the yardsticks tests/test_half_wave_shapes_gpu.py holds the three half-wave kernels to on skeletons other than SMPL's
(tests/skeleton_cases.py), and what of those shapes needs no device.

  * the fp64 restatements (tests/motion_ingest_model.py, motion_export_model.py) against an INDEPENDENT statement of the operation over the
    whole family: scipy.spatial.transform.Rotation composed parent -> child (ingest), parent^-1 child of the uprighted globals gathered by
    the inverse permutation written out here (export), an explicit per-body gather (the mirrored copy), export then ingest;
  * the conditions of the generated inputs: the 1e-3 floor on every decided sign, at most 1 redraw in 10 frames per case (so that the floor is no
    filter), the exact-zero band, and what ``settled`` removes;
  * joint_map and mirror_map are not their own inverse wherever J >= 3 (a kernel that applied the inverse map would otherwise pass);
  * the err_* yardsticks of profiles/half_wave_shapes.txt: max |model(float32) - model(float64)| over the family, floored at the golden fixture's
    figure for the same field -- recomputed here and compared with the stored figures, which are what the GPU test uses;
  * the launchers' bounds by name, at the edges of the body / history range, over made-up device addresses (nothing is launched)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import keypoint_stream_model as KM  # noqa: E402
import motion_export_model as MX  # noqa: E402
import motion_ingest_model as MI  # noqa: E402
import skeleton_cases as SC  # noqa: E402
from pulse_amd import _lib  # noqa: E402

AS_ROTATIONS = 1e-12                         # |q . q'| within this of 1: the same rotation to fp64 rounding
UPRIGHT = [0.5, 0.5, 0.5, 0.5]
INVALID = -1


def same_rotation(q, r):
    """1 - |q . r| over unit quaternions (q of the model, r a scipy Rotation)."""
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    return float((1.0 - np.abs((q * r.as_quat().reshape(q.shape)).sum(-1))).max())


def scipy_globals(c, poses):
    """from_rotvec of every body's SMPL joint (the hands zeroed), composed parent -> child: (frames, J) Rotations as a list per body."""
    aa = poses.astype(np.float64).reshape(len(poses), MI.SMPL_JOINTS, 3).copy()
    aa[:, MI.HAND_COL // 3:] = 0.0
    glob = []
    for b, p in enumerate(c["parents"]):
        local = Rotation.from_rotvec(aa[:, c["ingest_map"][b]])
        glob.append(local if p < 0 else glob[p] * local)
    return glob


# ------------------------------------------------------------------------------------------------------------------ the models vs scipy
@pytest.mark.parametrize("kind", SC.TREES)
def test_ingest_model_against_scipy_down_the_tree(kind):
    for c in SC.cases("ingest", kind):
        poses, trans, _ = SC.ingest_inputs(c)
        glob = scipy_globals(c, poses)
        plain, up = SC.ingest_model(c, poses, trans, upright_start=False), SC.ingest_model(c, poses, trans)
        turn = Rotation.from_quat(UPRIGHT).inv()
        for b in range(c["j"]):
            assert same_rotation(plain["pose_quat_global"][:, b], glob[b]) <= AS_ROTATIONS, (kind, c["j"], b)
            assert same_rotation(up["pose_quat_global"][:, b], glob[b] * turn) <= AS_ROTATIONS, (kind, c["j"], b)
        # the mirrored copy: body b takes the uprighted global of body mirror_map[b], x and z negated; the rest stays
        mirrored = SC.ingest_model(c, poses, trans, mirror=True)
        for b in range(c["j"]):
            want = up["pose_quat_global"][:, c["mirror_map"][b]] * np.array([-1.0, 1.0, -1.0, 1.0])
            assert np.array_equal(mirrored["pose_quat_global"][:, b], want), (kind, c["j"], b)
        assert np.array_equal(mirrored["root_trans_offset"], up["root_trans_offset"] * np.array([1.0, -1.0, 1.0]))
        for k in ("pose_quat", "pose_aa", "trans_orig"):
            assert np.array_equal(mirrored[k], up[k]), k
        assert np.array_equal(up["root_trans_offset"], trans.astype(np.float64) + SC.ROOT_OFFSET.astype(np.float64))
        assert np.array_equal(up["pose_aa"][:, :MI.HAND_COL], poses[:, :MI.HAND_COL].astype(np.float64)) and not up["pose_aa"][:, MI.HAND_COL:].any()


@pytest.mark.parametrize("kind", SC.TREES)
def test_export_model_against_scipy_local_rotations(kind):
    """pose_aa = as_rotvec(parent^-1 child) of the uprighted globals, in joint order.  The model rounds the local rotation to float32 as poselib
    does: up to 2^-24 per component of a unit quaternion, |dq| <= 2^-23 = 1.2e-7.  A rotation by an angle below pi moves by about 2 |dq| with it,
    and so does its vector, as long as the angle stays off pi, which the floor on w sees to: 2.4e-7 plus fp64 rounding, held here at 1e-6."""
    for c in SC.cases("export", kind):
        rb, dof, _ = SC.export_inputs(c)
        j = c["j"]
        rb, dof = rb.reshape(-1, j, 13), dof.reshape(len(rb.reshape(-1, j, 13)), 3 * (j - 1))
        res = SC.export_model(c, rb, dof)
        up = [Rotation.from_quat(rb[:, b, 3:7].astype(np.float64)) * Rotation.from_quat(UPRIGHT) for b in range(j)]
        local = [up[b] if p < 0 else up[p].inv() * up[b] for b, p in enumerate(c["parents"])]
        body_of_joint = [None] * j
        for b, s in enumerate(c["joint_map"]):                     # the inverse permutation, written out
            body_of_joint[s] = b
        want = np.concatenate([local[body_of_joint[s]].as_rotvec().reshape(-1, 3) for s in range(j)], axis=1)
        assert float(np.abs(res["pose_aa"] - want).max()) <= 1e-6, (kind, j)
        for b in range(j):
            assert same_rotation(res["upright"][:, b], up[b]) <= AS_ROTATIONS
        # with joint_map in place of its inverse the result is another one, by far more than any bound of the GPU test
        if j >= 3:
            swapped = MX.export_frames(rb, dof, c["parents"], SC.inverse(c["joint_map"]), root_offset=SC.ROOT_OFFSET)
            assert float(np.abs(swapped["pose_aa"] - res["pose_aa"]).max()) > 1e-2, (kind, j)
        # the copies and the dump
        assert np.array_equal(res["pose_quat_global"], rb[:, :, 3:7].astype(np.float64)) and np.array_equal(res["dof_pos"], dof.astype(np.float64))
        turn = Rotation.from_rotvec(dof.astype(np.float64).reshape(-1, 3)) if j > 1 else None
        if turn is not None:
            assert same_rotation(res["body_quat"][:, 1:].reshape(-1, 4), turn) <= AS_ROTATIONS


@pytest.mark.parametrize("kind", SC.TREES)
def test_export_then_ingest_returns_the_recording(kind):
    """The model of export, then the model of ingest on its pose_aa / trans_orig: the recording's normalised rotations up to sign and its root
    position, wherever the skeleton fits SMPL's 24 joints; bodies on the hand joints (which ingest zeroes) carry an identity local rotation."""
    hands = tuple(range(MI.HAND_COL // 3, MI.SMPL_JOINTS))
    ran = 0
    for c in SC.cases("export", kind):
        j = c["j"]
        if j > MI.SMPL_JOINTS:
            continue
        rb, dof, _ = SC.export_inputs(c, identity_joints=hands)
        rb, dof = rb.reshape(-1, j, 13), dof.reshape(len(rb.reshape(-1, j, 13)), 3 * (j - 1))
        out = SC.export_model(c, rb, dof)
        pose = np.zeros((len(rb), 3 * MI.SMPL_JOINTS))
        pose[:, :3 * j] = out["pose_aa"]
        back = MI.ingest_clip(pose, out["trans_orig"], 30.0, c["parents"], c["joint_map"], root_offset=SC.ROOT_OFFSET)
        src = MI.scipy_unit(rb[:, :, 3:7].astype(np.float64))
        assert float((1.0 - np.abs((back["pose_quat_global"] * src).sum(-1))).max()) < AS_ROTATIONS, (kind, j)
        assert float(np.abs(back["root_trans_offset"] - rb[:, 0, 0:3]).max()) < 1e-7
        ran += 1
    assert ran >= 1


# ------------------------------------------------------------------------------------------------------------------ the inputs' conditions
def _bounded(redraws, frames, what):
    assert 10 * (redraws["floor"] + redraws["band"]) <= frames, f"{what}: {redraws} redraws in {frames} frames: more than 1 in 10"


@pytest.mark.parametrize("kind", SC.TREES)
def test_floor_redraws_and_zero_band(kind):
    stored = SC.stored_yardsticks()
    for (kernel, field), (err, _, _) in stored.items():
        if kernel != "keypoint":
            assert 4 * err < SC.ZERO_BAND                        # the band covers what the GPU test's rule exempts from the sign comparison
    assert SC.RESIDUE * 1e6 < min(e for (k, _), (e, _, _) in stored.items() if e > 0)
    for c in SC.cases("ingest", kind):
        poses, trans, redraws = SC.ingest_inputs(c)
        assert poses.dtype == np.float32 and poses.shape == (SC.FRAMES, 72) and np.abs(poses[:, MI.HAND_COL:]).min() > 0
        _bounded(redraws, SC.FRAMES, f"ingest {kind} J = {c['j']}")
        hand_bodies = [b for b, s in enumerate(c["ingest_map"]) if s >= MI.HAND_COL // 3]
        for upright in (True, False):
            res = SC.ingest_model(c, poses, trans, upright_start=upright)
            assert (MI.decided_w(res) >= SC.W_FLOOR).all(), (kind, c["j"], upright)
            for f in ("pose_quat_global", "pose_quat", "root_trans_offset"):
                a = np.abs(SC.settled(res[f]))
                assert not ((a > 0) & (a < SC.ZERO_BAND)).any(), (kind, c["j"], f)
                # ``settled`` touches nothing but the vector part of an identity local rotation under the upright factor
                moved = np.argwhere(SC.settled(res[f]) != res[f])
                assert not len(moved) or (f == "pose_quat" and upright and set(moved[:, 1]) <= set(hand_bodies) and (moved[:, 2] < 3).all()), (kind, c["j"], f)
    for c in SC.cases("export", kind):
        rb, dof, redraws = SC.export_inputs(c)
        j = c["j"]
        assert rb.dtype == np.float32 and rb.shape == (SC.REC_STEPS, SC.REC_ENVS, j, 13) and dof.shape == (SC.REC_STEPS, SC.REC_ENVS, 3 * (j - 1))
        assert float(np.abs(np.linalg.norm(rb[..., 3:7].astype(np.float64), axis=-1) - 1).max()) < 1e-6      # unit rotations
        _bounded(redraws, SC.REC_STEPS * SC.REC_ENVS, f"export {kind} J = {j}")
        flat, dflat = rb.reshape(-1, j, 13), dof.reshape(SC.REC_STEPS * SC.REC_ENVS, 3 * (j - 1))
        for upright in (True, False):
            res = SC.export_model(c, flat, dflat, upright_start=upright)
            if upright:
                assert (MX.decided_w(res) >= SC.W_FLOOR).all(), (kind, j)
            assert (np.abs(res["body_quat"][..., 3]) >= SC.W_FLOOR).all() and (np.abs(res["pose_quat"][..., 3]) >= SC.W_FLOOR).all()
            for f in ("pose_quat", "pose_aa", "trans_orig", "body_quat"):
                a = np.abs(res[f])
                assert not ((a > 0) & (a < SC.ZERO_BAND)).any() and np.array_equal(SC.settled(res[f]), res[f]), (kind, j, f)
    for c, h, n, pushes in SC.keypoint_streams(kind):
        frames, redraws = SC.keypoint_frames(c, n, pushes)
        assert frames.shape == (pushes, n, c["j"], 3) and frames.dtype == np.float32
        _bounded(redraws, 10 * n, f"keypoint {kind} J = {c['j']} N = {n}")          # an env is drawn whole: at most one redraw per env
        p = frames.astype(np.float64)[:, :, c["joint_map"]]
        for i in range(1, KM.LIMBS + 1):
            assert float(np.linalg.norm(p[:, :, c["parents"][i]] - p[:, :, i], axis=-1).min()) >= SC.MIN_LIMB


def depth(par):
    d = [0] * len(par)
    for b in range(1, len(par)):
        d[b] = d[par[b]] + 1
    return max(d)


def test_the_family_holds_the_shapes():
    assert SC.body_counts("ingest", "chain") == (1, 2, 6, 23, 25, 31, 32) and SC.body_counts("export", "star") == (2, 6, 23, 25, 31, 32)
    assert SC.body_counts("keypoint", "late_low") == (6, 7, 30, 31) and SC.body_counts("export", "smpl") == (24,)
    assert SC.parents_of("chain", 4) == [-1, 0, 1, 2] and SC.parents_of("star", 4) == [-1, 0, 0, 0] and SC.parents_of("late_low", 6) == [-1, 0, 1, 2, 0, 1]
    assert depth(SC.parents_of("chain", 32)) == 31 and depth(SC.parents_of("star", 32)) == 1 and depth(SC.parents_of("late_low", 32)) == 29
    for kernel in SC.KERNELS:
        for kind in SC.TREES:
            for c in SC.cases(kernel, kind):
                par, j = c["parents"], c["j"]
                assert par[0] == -1 and all(0 <= par[b] < b for b in range(1, j))
                if kind == "random" and j >= 23:
                    assert 1 < depth(par) < j - 1                   # neither a star nor a chain
                for name in ("joint_map", "mirror_map"):
                    assert sorted(c[name]) == list(range(j))
                    if kind != "smpl" and j >= 3:                  # not its own inverse: the inverse map gives another result
                        assert c[name] != SC.inverse(c[name]), (kernel, kind, j, name)
                if j > MI.SMPL_JOINTS:
                    assert sorted(set(c["ingest_map"])) == list(range(MI.SMPL_JOINTS)) and max(c["ingest_map"][MI.SMPL_JOINTS:]) < MI.HAND_COL // 3
                else:
                    assert len(set(c["ingest_map"])) == j
    smpl = SC.case("ingest", "smpl", 24)
    assert smpl["mirror_map"] == SC.inverse(smpl["mirror_map"])      # the control IS an involution: what the fixtures could not tell apart


# ------------------------------------------------------------------------------------------------------------------ the yardsticks
# numpy takes float32 sin / cos / arctan2 / arccos from the CPU's vector library where there is one and from libm elsewhere; the two may round
# the element that sets a maximum differently, by one float32 step at that field's magnitude (rotation vectors and metres below 8: 2^-21 at
# most, usually 2^-22; unit quaternion components: 2^-24).  The stored figure is the one the GPU test uses, whichever machine recomputes it.
STEP = {"pose_aa": 2.0 ** -22, "root_trans_offset": 2.0 ** -22, "trans_orig": 2.0 ** -22, "pos": 2.0 ** -22, "vel": 2.0 ** -17}


def test_stored_yardsticks_are_the_family_maximum_over_the_fixture_floor():
    fresh, stored, fixture = SC.yardsticks(), SC.stored_yardsticks(), SC.fixture_err()
    assert set(fresh) == set(stored) == {(k, f) for k in SC.KERNELS for f in SC.FIELDS[k]}
    for key, (err, source) in fresh.items():
        print(f"{key[0]} {key[1]}: recomputed {err!r} ({source}); stored {stored[key][0]!r} ({stored[key][1]}); fixture {fixture[key]!r}")
    for key, (err, source) in fresh.items():
        got, src, _ = stored[key]
        assert src == source, key
        if source == "fixture":
            assert got == fixture[key], key
        else:
            assert got > fixture[key] and abs(got - err) <= STEP.get(key[1], 2.0 ** -24), (key, got, err)
    for kernel in SC.KERNELS:
        for f in SC.COPIES[kernel]:
            assert stored[kernel, f][0] == 0.0                    # copies: exact in every precision


# ------------------------------------------------------------------------------------------------------------------ launcher bounds, by name
def _tables(j):
    keep = {"a": torch.tensor([0, 1], dtype=torch.int64), "b": torch.tensor([1, 1], dtype=torch.int64), "frames": torch.tensor([3, 2], dtype=torch.int64),
            "par": (ctypes.c_int32 * max(j, 1))(*range(-1, max(j, 1) - 1))}
    return keep


def _ingest_args(j):
    """An argument struct the launcher would accept for a chain of j bodies, over made-up device addresses (every case breaks one thing)."""
    keep = _tables(min(j, 32))
    a = _lib.MotionIngestArgs()
    for i, name in enumerate(("src_pose", "src_trans", "clip_src_start", "clip_skip", "clip_out_start", "out_rot", "out_trans")):
        setattr(a, name, 4096 * (i + 1))
    a.src_frames, a.num_clips, a.num_bodies, a.total_frames = 8, 2, j, 5
    a.clip_src_start_host, a.clip_skip_host, a.clip_frames_host = keep["a"].data_ptr(), keep["b"].data_ptr(), keep["frames"].data_ptr()
    a.parent_indices_host = ctypes.cast(keep["par"], ctypes.c_void_p)
    for b in range(min(j, 32)):
        a.joint_map[b], a.mirror_map[b] = b % MI.SMPL_JOINTS, b
    return a, keep


def _export_args(j):
    keep = _tables(min(j, 32))
    a = _lib.MotionExportArgs()
    for i, name in enumerate(("rb", "dof_pos", "seg_env", "seg_t0", "seg_out_start", "out_rot", "out_trans")):
        setattr(a, name, 4096 * (i + 1))
    a.rb_stride_t, a.rb_stride_n, a.rb_stride_b, a.dof_stride_t, a.dof_stride_n = 2 * j * 13, j * 13, 13, 2 * 3 * (j - 1), 3 * (j - 1)
    a.num_steps, a.num_envs, a.num_bodies, a.num_segments, a.total_frames, a.upright_start = 4, 2, j, 2, 5, 1
    a.seg_env_host, a.seg_t0_host, a.seg_frames_host = keep["a"].data_ptr(), keep["b"].data_ptr(), keep["frames"].data_ptr()
    a.parent_indices_host = ctypes.cast(keep["par"], ctypes.c_void_p)
    for b in range(min(j, 32)):
        a.joint_map[b] = b
    return a, keep


def _keypoint_args(j, history=30):
    a = _lib.KeypointPushArgs()
    a.num_envs, a.num_bodies, a.history, a.dt = 1, j, history, 1 / 30
    a.j3d_stride_n, a.j3d_stride_j = 3 * j, 3
    for b in range(min(j, 32)):
        a.joint_map[b], a.parent_indices[b] = b, b - 1
    for f in ("j3d", "taps", "root_ring", "body_ring", "count", "prev_pos", "pos", "vel"):
        setattr(a, f, 64)                                         # never dereferenced: every case fails a check first
    return a, None


def _break(a, keep, what):
    if what == "tree_last":                                       # parent == child at the last body
        j = a.num_bodies
        if keep is None:
            a.parent_indices[j - 1] = j - 1
        else:
            keep["par"][j - 1] = j - 1
    elif what == "map_twice":
        a.joint_map[31] = a.joint_map[7]
    elif what == "mirror_is_J":
        a.mirror_map[5] = a.num_bodies


BOUNDS = [("pulse_motion_ingest", _ingest_args, 0, None, "num_bodies 0 not in [1,32]"), ("pulse_motion_ingest", _ingest_args, 33, None, "num_bodies 33 not in [1,32]"),
          ("pulse_motion_export", _export_args, 0, None, "num_bodies 0 not in [1,32]"), ("pulse_motion_export", _export_args, 33, None, "num_bodies 33 not in [1,32]"),
          ("pulse_keypoint_push", _keypoint_args, 5, None, "num_bodies 5 not in [6,31]"), ("pulse_keypoint_push", _keypoint_args, 32, None, "num_bodies 32 not in [6,31]"),
          ("pulse_keypoint_push", lambda j: _keypoint_args(j, 0), 31, None, "history 0 not in [1,64]"),
          ("pulse_keypoint_push", lambda j: _keypoint_args(j, 65), 6, None, "history 65 not in [1,64]"),
          ("pulse_motion_export", _export_args, 32, "map_twice", "joint_map[31] = 7 is taken twice"),
          ("pulse_motion_ingest", _ingest_args, 32, "mirror_is_J", "mirror_map[5] = 32 is no body (0 .. 31)"),
          ("pulse_motion_ingest", _ingest_args, 32, "tree_last", "parent_indices[31] = 31: every parent must precede its child"),
          ("pulse_motion_export", _export_args, 32, "tree_last", "parent_indices[31] = 31: every parent must precede its child"),
          ("pulse_keypoint_push", _keypoint_args, 31, "tree_last", "parent_indices[30] = 30: every parent must precede its child")]


@pytest.mark.parametrize("entry,make,j,what,needle", BOUNDS, ids=[f"{b[0][6:]}-{b[2]}-{b[3] or b[4].split()[0]}-{i}" for i, b in enumerate(BOUNDS)])
def test_bounds_are_refused_by_name(entry, make, j, what, needle):
    lib = _lib.load()
    a, keep = make(j)
    if what is None:                                              # the struct as made is at the bound ...
        pass
    else:                                                         # ... or is accepted up to the launch, and then broken in one place
        _break(a, keep, what)
    rc = getattr(lib, entry)(ctypes.byref(a), None)
    msg = lib.pulse_last_error().decode()
    assert rc == INVALID and needle in msg and msg.startswith(entry + ": "), (rc, msg)
