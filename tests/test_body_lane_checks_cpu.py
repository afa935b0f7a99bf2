"""No device: the host checks the launchers of the body-lane kernels share (pulse_amd/csrc/body_lanes.h) -- check_motion_tables from its four
consumers, check_tree from its four users, check_permutation from its two.  Argument structs over made-up addresses, one thing broken per case:
every case is refused with PULSE_ERR_INVALID_ARG before anything is launched, and apart from the entry point's name in front the message is the
same string whichever entry point met the fault.

J = 3 throughout: the smallest skeleton reaches every branch.  pulse_keypoint_push takes 6 bodies, the fewest it accepts (bodies 1 .. 5 are its
limbs).  The body-count bound is the one case whose text is the entry's own: the widest lane group differs (64 | 32), and
pulse_task_ref_state_init keeps its lower bound of 2 bodies in front of the shared check."""
import ctypes

import pytest
import torch

from pulse_amd import _lib
from pulse_amd.env.motion_lib import MotionLib

INVALID = -1
J = 3
OFFSETS, STRIDE, WIDTHS = MotionLib.record_layout(J)
BASE = 1 << 20                                  # made-up, 16-byte aligned addresses: nothing is dereferenced


def _tables(t):
    t.frames, t.frame_stride, t.total_frames, t.num_bodies, t.num_motions = BASE, STRIDE, 8, J, 2
    for k, v in OFFSETS.items():
        setattr(t, "off_" + k, v)
    for i, name in enumerate(("motion_lengths", "motion_dt", "motion_num_frames", "length_starts")):
        setattr(t, name, BASE + 4096 * (i + 1))


def _motion_state():
    a = _lib.MotionStateArgs()
    _tables(a.tab)
    a.n, a.motion_ids, a.motion_times = 4, BASE + 65536, BASE + 69632
    return a, a.tab, None


def _im_step():
    a = _lib.ImStepArgs()
    _tables(a.motion)
    width = _lib.load().pulse_self_obs_width_ex(J, 1, 1, 1, 0)
    a.what, a.rb, a.rb_env_stride, a.num_envs, a.num_bodies, a.time_steps = _lib.PULSE_IM_SELF_OBS, BASE + 65536, 13 * J, 4, J, 1
    a.self_obs_version, a.hist_steps, a.obs_version, a.root_height_obs = 1, 1, 6, 1
    a.obs, a.obs_cols, a.obs_stride = BASE + 131072, width, width
    a.use_motion, a.motion_ids, a.progress, a.clock_dt = 1, BASE + 69632, BASE + 73728, 1 / 30
    return a, a.motion, None


def _amp_hist():
    a = _lib.AmpHistArgs()
    _tables(a.tab)
    a.num_envs, a.hist_steps = 4, 2
    return a, a.tab, None


def _task_reset():
    a = _lib.TaskResetArgs()
    _tables(a.tab)
    a.num_envs = 4
    return a, a.tab, None


# entry point -> (a struct its launcher would take as far as the tables, the widest lane group, the fewest bodies it names)
TABLE_USERS = {"pulse_motion_state": (_motion_state, 64, 1), "pulse_im_step": (_im_step, 64, 1), "pulse_amp_hist_init": (_amp_hist, 32, 1),
               "pulse_task_ref_state_init": (_task_reset, 32, 2)}
POINTERS = ("frames", "motion_lengths", "motion_dt", "motion_num_frames", "length_starts")
FIELDS = ("off_gts", "off_grs", "off_lrs", "off_gvs", "off_gavs", "off_dvs")
PAST = STRIDE - WIDTHS["dvs"] + 1                # dof velocities ending one float behind the record

TABLE_CASES = [("null_" + p, lambda t, p=p: setattr(t, p, None), f"null table pointer ({p})") for p in POINTERS]
TABLE_CASES += [("no_motions", lambda t: setattr(t, "num_motions", 0), "num_motions 0: the motion tables hold no clip"),
                ("stride_6", lambda t: setattr(t, "frame_stride", 6),
                 "frame_stride 6 is no multiple of 4 floats: the record pitch and the quaternion fields must start on 16-byte boundaries"),
                ("off_lrs_2", lambda t: setattr(t, "off_lrs", 2), "off_lrs 2 is no multiple of 4 floats: the record pitch and the quaternion fields must start on 16-byte boundaries")]
TABLE_CASES += [(f + "_negative", lambda t, f=f: setattr(t, f, -4), f"negative field offset ({f} -4)") for f in FIELDS]
TABLE_CASES += [("dvs_past_stride", lambda t: setattr(t, "off_dvs", PAST), f"off_dvs {PAST}: its {WIDTHS['dvs']} floats end past frame_stride {STRIDE}"),
                ("frames_misaligned", lambda t: setattr(t, "frames", BASE + 4), "frames (the record base) must be 16-byte aligned")]


def _refused(entry, a, message):
    lib = _lib.load()
    rc = getattr(lib, entry)(ctypes.byref(a), None)
    got = lib.pulse_last_error().decode()
    assert rc == INVALID and got == f"{entry}: {message}", (entry, rc, got)


@pytest.mark.parametrize("entry", list(TABLE_USERS))
@pytest.mark.parametrize("what,change,message", TABLE_CASES, ids=[c[0] for c in TABLE_CASES])
def test_motion_tables_refused_alike(entry, what, change, message):
    a, tab, _ = TABLE_USERS[entry][0]()
    change(tab)
    _refused(entry, a, message)


@pytest.mark.parametrize("entry", list(TABLE_USERS))
@pytest.mark.parametrize("bodies", ["none", "one_too_many"])
def test_motion_tables_body_count(entry, bodies):
    make, most, fewest = TABLE_USERS[entry]
    a, tab, _ = make()
    tab.num_bodies = 0 if bodies == "none" else most + 1
    own = " (a 32-lane half-wave per env, lane = body)" if fewest == 2 else ""      # the entry's own check in front of the shared one
    _refused(entry, a, f"num_bodies {tab.num_bodies} not in [{fewest},{most}]{own}")


# ------------------------------------------------------------------------------------------------------------------ tree and permutation
def _spread(a, names):
    for i, name in enumerate(names):
        setattr(a, name, BASE + 4096 * i)


def _motion_build():
    keep = {"frames": torch.tensor([2, 3], dtype=torch.int64), "par": (ctypes.c_int32 * J)(-1, 0, 1)}
    a = _lib.MotionBuildArgs()
    _spread(a, ("src_rot", "src_trans", "clip_src_start", "clip_out_start", "clip_dt", "local_translation", "frames"))
    a.src_frames, a.num_clips, a.num_bodies, a.total_frames, a.frame_stride = 5, 2, J, 5, STRIDE
    for k, v in OFFSETS.items():
        setattr(a, "off_" + k, v)
    a.clip_frames_host, a.parent_indices_host = keep["frames"].data_ptr(), ctypes.cast(keep["par"], ctypes.c_void_p)
    return a, keep["par"], keep


def _motion_ingest():
    keep = {"start": torch.tensor([0, 6], dtype=torch.int64), "skip": torch.tensor([2, 1], dtype=torch.int64),
            "frames": torch.tensor([3, 2], dtype=torch.int64), "par": (ctypes.c_int32 * J)(-1, 0, 1)}
    a = _lib.MotionIngestArgs()
    _spread(a, ("src_pose", "src_trans", "clip_src_start", "clip_skip", "clip_out_start", "out_rot", "out_trans"))
    a.src_frames, a.num_clips, a.num_bodies, a.total_frames = 8, 2, J, 5
    a.clip_src_start_host, a.clip_skip_host, a.clip_frames_host = keep["start"].data_ptr(), keep["skip"].data_ptr(), keep["frames"].data_ptr()
    a.parent_indices_host = ctypes.cast(keep["par"], ctypes.c_void_p)
    a.joint_map[:J], a.mirror_map[:J] = [0, 2, 3], [0, 2, 1]
    return a, keep["par"], keep


def _motion_export():
    keep = {"env": torch.tensor([0, 1], dtype=torch.int64), "t0": torch.tensor([0, 2], dtype=torch.int64),
            "frames": torch.tensor([3, 2], dtype=torch.int64), "par": (ctypes.c_int32 * J)(-1, 0, 1)}
    a = _lib.MotionExportArgs()
    _spread(a, ("rb", "dof_pos", "seg_env", "seg_t0", "seg_out_start", "out_rot", "out_trans"))
    a.rb_stride_t, a.rb_stride_n, a.rb_stride_b, a.dof_stride_t, a.dof_stride_n = 2 * J * 13, J * 13, 13, 2 * 3 * (J - 1), 3 * (J - 1)
    a.num_steps, a.num_envs, a.num_bodies, a.num_segments, a.total_frames, a.upright_start = 4, 2, J, 2, 5, 1
    a.seg_env_host, a.seg_t0_host, a.seg_frames_host = keep["env"].data_ptr(), keep["t0"].data_ptr(), keep["frames"].data_ptr()
    a.parent_indices_host = ctypes.cast(keep["par"], ctypes.c_void_p)
    a.joint_map[:J] = [0, 2, 1]
    return a, keep["par"], keep


KP = 6


def _keypoint_push():
    a = _lib.KeypointPushArgs()
    a.num_envs, a.num_bodies, a.history, a.dt = 1, KP, 30, 1 / 30
    a.j3d_stride_n, a.j3d_stride_j = 3 * KP, 3
    a.joint_map[:KP] = [0, 2, 1, 4, 3, 5]
    a.parent_indices[:KP] = [-1, 0, 1, 2, 3, 4]
    for f in ("j3d", "taps", "root_ring", "body_ring", "count", "prev_pos", "pos", "vel"):
        setattr(a, f, BASE)
    return a, a.parent_indices, None


TREE_USERS = {"pulse_motion_build": _motion_build, "pulse_motion_ingest": _motion_ingest, "pulse_motion_export": _motion_export,
              "pulse_keypoint_push": _keypoint_push}
TREE_CASES = [(0, 0, "body 0 must be the root (parent -1), got parent 0"),
              (2, 2, "parent_indices[2] = 2: every parent must precede its child (0 <= parent < child)"),
              (1, -1, "parent_indices[1] = -1: every parent must precede its child (0 <= parent < child)")]


@pytest.mark.parametrize("entry", list(TREE_USERS))
@pytest.mark.parametrize("body,parent,message", TREE_CASES, ids=["root_with_parent", "own_parent", "second_root"])
def test_tree_refused_alike(entry, body, parent, message):
    a, parents, keep = TREE_USERS[entry]()
    parents[body] = parent
    _refused(entry, a, message)


@pytest.mark.parametrize("entry,make,bodies", [("pulse_motion_export", _motion_export, J), ("pulse_keypoint_push", _keypoint_push, KP)])
@pytest.mark.parametrize("case", ["out_of_range", "repeated"])
def test_permutation_refused_alike(entry, make, bodies, case):
    a, _, keep = make()
    if case == "out_of_range":
        a.joint_map[1] = bodies
        message = f"joint_map[1] = {bodies} is no SMPL joint (0 .. {bodies - 1})"
    else:
        a.joint_map[2] = a.joint_map[0]
        message = f"joint_map[2] = {a.joint_map[0]} is taken twice: joint_map must be a permutation of 0 .. {bodies - 1}"
    _refused(entry, a, message)
