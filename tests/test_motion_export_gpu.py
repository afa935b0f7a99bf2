"""GPU: pulse_motion_export against the reference's own statements (tests/golden/motion_export.npz, tools/gen_golden_motion_export.py) and the fp64
restatement (tests/motion_export_model.py), and the host side on top of it (segment_recording, export_motion, CommonPlayer.generate_motion).

Per output field, over every element, the rule of tests/test_motion_ingest_gpu.py:

    sign(hip) == sign(expected)   and   |hip - expected| <= 4 * err_field

with ``expected`` the reference's fp64 run and ``err_field`` the distance of the reference's OWN fp32 run from it (max over the fixture, stored in
it).  The sign is compared on every component larger than the bound, the only expected components below it must be exact zeros (asserted), and every
quaternion as a whole must be q, not -q.  out_rot, out_trans and out_dof_pos are copies: bit for bit.  The figures are printed before they are asserted.

The kernel runs on the fixture's 7 x 9 recording: 21 segments, 63 output frames = 7.875 workgroups of eight, 24 of 32 lanes per frame; ``rb`` and
``dof_pos`` are strided views of larger NaN-filled buffers.  Every output sits between poison-filled guard rows that must come back untouched.
``upright_start=False`` has no runnable counterpart over whole recordings in the reference: it is held to the model, at the same bounds.

Round trip: kernels.motion_ingest on the export's pose_aa / trans_orig against the reference's own round trip (render()'s chain, then the loop body of
convert_amass_isaac.py) in fp64, at 4 x the distance of its fp32-staged run -- every body of every round-trip frame (the frames whose hands are identity:
ingest zeroes the hand joints)."""
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

import gen_golden_motion_export as GX  # noqa: E402
import motion_export_model as MX  # noqa: E402
from pulse_amd import configs, kernels  # noqa: E402
from pulse_amd import synthetic as syn  # noqa: E402
from pulse_amd._lib import PulseLibraryError  # noqa: E402
from pulse_amd.env import motion_export as ME  # noqa: E402
from pulse_amd.env.motion_lib import MotionLib  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 3                                    # poison rows before and after every output
POISON = 0x7FC0DEAD                          # a NaN with a payload: any write shows
OUT = {"out_rot": (24, 4), "out_trans": (3,), "out_pose_quat": (24, 4), "out_pose_aa": (72,), "out_trans_orig": (3,), "out_body_quat": (24, 4),
       "out_dof_pos": (69,)}
FIELD_OF = {"out_rot": "pose_quat_global", "out_trans": "root_trans_offset", "out_pose_quat": "pose_quat", "out_pose_aa": "pose_aa",
            "out_trans_orig": "trans_orig", "out_body_quat": "body_quat", "out_dof_pos": "dof_pos"}
GOLDEN_OF = {"body_quat": "states_body_quat", "dof_pos": "states_dof_pos"}
COPIES = ("out_rot", "out_trans", "out_dof_pos")


@pytest.fixture(scope="module")
def fx():
    return GX.load()


def strided(dev, a, pad):
    """``a`` as a view into a larger NaN-filled device buffer: ``pad`` = per dimension (before, after)."""
    big = torch.full([s + p + q for s, (p, q) in zip(a.shape, pad)], float("nan"), device=dev)
    view = big[tuple(slice(p, p + s) for s, (p, _) in zip(a.shape, pad))]
    view.copy_(torch.from_numpy(a))
    assert not view.is_contiguous()
    return view


def export(dev, fx, segs, outputs=tuple(OUT), dof=True, upright_start=True):
    """The kernel on ``segs`` [(env, t0, frames)] of the fixture's recording -> outputs with their guard rows (CPU)."""
    rb = strided(dev, fx["rb"], [(1, 1), (2, 1), (1, 1), (0, 3)])
    dof_pos = strided(dev, fx["dof_pos"], [(1, 0), (1, 1), (0, 3)]) if dof else None
    total = sum(s[2] for s in segs)
    full = {k: torch.full((total + 2 * GUARD,) + OUT[k], POISON, dtype=torch.int32, device=dev).view(torch.float32) for k in outputs}
    view = {k: v[GUARD:GUARD + total] for k, v in full.items()}
    table = lambda i: torch.tensor([s[i] for s in segs], dtype=torch.int64)
    kernels.motion_export(view["out_rot"], view["out_trans"], rb=rb, dof_pos=dof_pos, seg_env=table(0), seg_t0=table(1), seg_frames=table(2),
                          parents=syn.SMPL_PARENTS, joint_map=syn.smpl_joint_map(), upright_start=upright_start, root_offset=fx["root_offset"].tolist(),
                          **{k: v for k, v in view.items() if k not in ("out_rot", "out_trans")})
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in full.items()}


def model(fx, segs, **kw):
    frames, dofs = MX.gather(fx["rb"], fx["dof_pos"], segs)
    return MX.export_frames(frames, dofs, syn.SMPL_PARENTS, syn.smpl_joint_map(), root_offset=fx["root_offset"], **kw)


def held(got, want, err, name):
    """sign and value of ``got`` (fp32) against ``want`` (fp64) at 4 x err (module docstring); the figure is printed first."""
    got = np.asarray(got).astype(np.float64).reshape(want.shape)
    worst = float(np.abs(got - want).max())
    print(f"{name}: max |hip - expected| {worst:.3e} = {worst / err if err else 0.0:.2f} x err ({err:.3e})")
    assert np.isfinite(got).all(), name
    carries = np.abs(want) > 4 * err
    assert not want[~carries].any(), f"{name}: an expected component within the bound of zero is not exactly zero"    # the exempt set cannot grow unnoticed
    assert np.array_equal(np.sign(got[carries]), np.sign(want[carries])), f"{name}: a sign differs"
    if want.shape[-1] == 4:
        assert ((got * want).sum(-1) > 0).all(), f"{name}: a quaternion came out as -q"
    assert worst <= 4 * err, f"{name}: {worst:.3e} > 4 x {err:.3e}"
    return worst


def err_of(fx, field):
    return float(fx["err_" + GOLDEN_OF.get(field, field)])


def body(full, k, total):
    return full[k][GUARD:GUARD + total].numpy()


@pytest.fixture(scope="module")
def plain(dev, fx):
    return export(dev, fx, GX.segs_of(fx))


def test_kernel_against_golden_and_model(fx, plain):
    segs = GX.segs_of(fx)
    assert len(segs) == 21 and sum(s[2] for s in segs) == 63
    res = model(fx, segs)
    for k, field in FIELD_OF.items():
        got = body(plain, k, 63)
        held(got, fx[GOLDEN_OF.get(field, field)], err_of(fx, field), f"{field} vs golden")
        held(got, res[field], err_of(fx, field), f"{field} vs model")
    frames, dofs = MX.gather(fx["rb"], fx["dof_pos"], segs)
    for k, src in (("out_rot", frames[:, :, 3:7]), ("out_trans", frames[:, 0, 0:3]), ("out_dof_pos", dofs)):            # copies: bit for bit
        assert np.array_equal(body(plain, k, 63).view(np.int32), np.ascontiguousarray(src).view(np.int32).reshape(body(plain, k, 63).shape)), k


def test_guard_rows_stay_poisoned(plain):
    for k, t in plain.items():
        bits = t.view(torch.int32)
        assert (bits[:GUARD] == POISON).all() and (bits[GUARD + 63:] == POISON).all(), f"{k}: a guard row was written"
        assert not (bits[GUARD:GUARD + 63] == POISON).any(), f"{k}: an output element was not written"


def test_without_upright_start_against_the_model(dev, fx):
    segs = GX.segs_of(fx)
    full = export(dev, fx, segs, upright_start=False)
    res = model(fx, segs, upright_start=False)
    for k, field in FIELD_OF.items():
        held(body(full, k, 63), res[field], err_of(fx, field), f"{field}, no upright factor, vs model")
    assert torch.equal(full["out_pose_quat"].view(torch.int32), full["out_body_quat"].view(torch.int32))      # [root quat, exp_map_to_quat(dof_pos)], both
    up = model(fx, segs)
    assert np.array_equal(res["body_quat"], up["body_quat"])


def test_subsets_of_segments_and_outputs(dev, fx, plain):
    segs = GX.segs_of(fx)
    # one frame in all: a one-frame segment in the middle of an env
    one = [s for s in segs if s[2] == 1][1:2]
    full = export(dev, fx, one)
    at = sum(s[2] for s in segs[:segs.index(one[0])])
    for k in OUT:
        assert torch.equal(full[k][GUARD:GUARD + 1].view(torch.int32), plain[k][GUARD + at:GUARD + at + 1].view(torch.int32)), k
        assert (full[k].view(torch.int32)[:GUARD] == POISON).all() and (full[k].view(torch.int32)[GUARD + 1:] == POISON).all(), k
    # zero segments: nothing is launched, nothing is written
    full = export(dev, fx, [])
    assert all((v.view(torch.int32) == POISON).all() for v in full.values())
    # out_pose_aa alone; dof_pos absent (the outputs that need it are refused, the others are the bits of the full run)
    order = [segs[i] for i in (5, 0, 20, 9)]                                  # and segments in another order than the recording's
    sub = export(dev, fx, order, outputs=("out_rot", "out_trans", "out_pose_aa"), dof=False)
    pos = 0
    for s in order:
        at = sum(x[2] for x in segs[:segs.index(s)])
        for k in ("out_rot", "out_trans", "out_pose_aa"):
            assert torch.equal(sub[k][GUARD + pos:GUARD + pos + s[2]].view(torch.int32), plain[k][GUARD + at:GUARD + at + s[2]].view(torch.int32)), (s, k)
        pos += s[2]
    for k in sub:
        bits = sub[k].view(torch.int32)
        assert (bits[:GUARD] == POISON).all() and (bits[GUARD + pos:] == POISON).all(), k
    with pytest.raises(PulseLibraryError, match="out_body_quat / out_dof_pos need dof_pos"):
        export(dev, fx, segs[:2], outputs=("out_rot", "out_trans", "out_body_quat"), dof=False)
    with pytest.raises(PulseLibraryError, match="without upright_start out_pose_quat / out_pose_aa need dof_pos"):
        export(dev, fx, segs[:2], outputs=("out_rot", "out_trans", "out_pose_aa"), dof=False, upright_start=False)
    with pytest.raises(PulseLibraryError, match="segment 0 reads 7 steps from 1"):
        export(dev, fx, [(0, 1, 7)])


def test_round_trip_through_ingest(dev, fx, plain):
    sel = fx["roundtrip_frames"]
    n = len(sel)
    assert sel.tolist() == list(range(n)) and n == 42
    pose_aa = plain["out_pose_aa"][GUARD:GUARD + n].contiguous().to(dev)
    trans = plain["out_trans_orig"][GUARD:GUARD + n].contiguous().to(dev)
    rot, back = torch.empty(n, 24, 4, device=dev), torch.empty(n, 3, device=dev)
    kernels.motion_ingest(rot, back, src_pose=pose_aa, src_trans=trans, clip_src_start=torch.tensor([0]), clip_skip=torch.tensor([1]),
                          clip_frames=torch.tensor([n]), parents=syn.SMPL_PARENTS, joint_map=syn.smpl_joint_map(), root_offset=fx["root_offset"].tolist())
    torch.cuda.synchronize()
    held(rot.cpu().numpy(), fx["roundtrip_pose_quat_global"], float(fx["err_roundtrip_pose_quat_global"]), "round trip pose_quat_global (every body, every frame)")
    held(back.cpu().numpy(), fx["roundtrip_root_trans_offset"], float(fx["err_roundtrip_root_trans_offset"]), "round trip root_trans_offset")
    # and what comes back IS what went out: the recorded rotation up to its sign and norm, the recorded root position
    src = plain["out_rot"][GUARD:GUARD + n].double().numpy()
    src = src / np.linalg.norm(src, axis=-1, keepdims=True)
    q = rot.cpu().double().numpy()
    gap = float(np.minimum(np.abs(q - src).max(-1), np.abs(q + src).max(-1)).max())
    print(f"round trip: largest |q_out - (+-)q_recorded| {gap:.3e}")
    # (the reference's fp64 round trip is the normalised recording up to its sign to 1e-12: tests/test_motion_export_cpu.py)
    assert gap <= 4 * float(fx["err_roundtrip_pose_quat_global"]) + 1e-12
    assert torch.equal(back.cpu(), plain["out_trans"][GUARD:GUARD + n])


def test_segment_recording_on_the_device(dev, fx):
    for rec in [fx["progress"]] + [np.asarray(r) for r in MX.EDGE_RECORDINGS]:
        got = ME.segment_recording(torch.as_tensor(rec, dtype=torch.int64).to(dev))
        want = MX.segments(rec)
        assert list(zip(got["env"].tolist(), got["t0"].tolist(), got["frames"].tolist())) == want and got["keys"] == MX.segment_keys(want)
        assert all(v.device.type == "cpu" for v in (got["env"], got["t0"], got["frames"]))


def test_export_motion_forms(dev, fx):
    rb, dof, prog = (torch.from_numpy(fx[k]).to(dev) for k in ("rb", "dof_pos", "progress"))
    trees = (syn.SMPL_PARENTS, torch.zeros(2, 24, 3) + torch.from_numpy(fx["root_offset"]))                 # local_translation[0] of slot 0 is the offset
    motion = ME.export_motion(rb, prog, trees, dof_pos=dof, dt=1 / 30)
    assert list(motion) == fx["keys"].tolist() and not motion.dropped
    at = 0
    for key, n in zip(motion, GX.SEGMENT_FRAMES):
        clip = motion[key]
        assert set(clip) == {"pose_quat_global", "pose_quat", "trans_orig", "root_trans_offset", "beta", "gender", "pose_aa", "fps"}
        assert clip["fps"] == 30 and clip["gender"] == "neutral" and not clip["beta"].any() and clip["pose_aa"].shape == (n, 72)
        for field in GX.FIELDS:
            held(clip[field], fx[field][at:at + n], err_of(fx, field), f"export_motion {key} {field}")
        at += n
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        shapes = torch.arange(9 * 17, dtype=torch.float32).reshape(9, 17)
        states = ME.export_motion(rb, prog, trees, dof_pos=dof, fps=60, form="states", min_frames=2, betas=shapes)
    told = [str(w.message) for w in caught if "export_motion" in str(w.message)]
    short = [k for k, n in zip(fx["keys"].tolist(), GX.SEGMENT_FRAMES) if n < 2]
    assert len(told) == 1 and all(k in told[0] for k in short) and f"dropped {len(short)} segment(s)" in told[0]
    assert [k for k, _ in states.dropped] == short and states.dropped_frames == len(short) and list(states) == [k for k in fx["keys"].tolist() if k not in short]
    at = 0
    for key, n in zip(fx["keys"].tolist(), GX.SEGMENT_FRAMES):
        if key in states:
            clip = states[key]
            assert set(clip) == {"body_quat", "trans", "root_states_seg", "dof_pos", "fps", "betas"} and clip["fps"] == 60
            assert np.array_equal(clip["betas"], shapes[int(key.split("_")[0])].numpy())
            for field in GX.STATE_FIELDS:
                held(clip[field], fx["states_" + field][at:at + n], float(fx["err_states_" + field]), f"export_motion states {key} {field}")
        at += n
    with pytest.raises(ValueError, match="needs dof_pos"):
        ME.export_motion(rb, prog, trees, fps=60, form="states")
    shaped = ME.export_motion(rb, prog, trees, dof_pos=dof, fps=30, betas=shapes)                          # beta: 16 long with or without betas
    for key, clip in shaped.items():
        e = int(key.split("_")[0])
        assert clip["beta"].shape == (16,) and np.array_equal(clip["beta"][:10], shapes[e, 1:11].numpy()) and not clip["beta"][10:].any()
        assert np.array_equal(clip["pose_aa"], motion[key]["pose_aa"])


def test_generate_motion_end_to_end(dev):
    steps, envs = 12, 8
    player = configs.make_player("cfg3_small", device=str(dev), z_source="prior", num_envs_override=envs, minibatch_size=16 * envs)     # (horizon 16)
    before = player.generate(3, record=True)
    assert set(before) == {"rb", "z", "steps", "resets"} and before["rb"].shape[:2] == (3, envs)          # generate: the keys it returned before
    counted = []
    inner = kernels._launch
    kernels._launch = lambda name, *a, **k: (counted.append(name), inner(name, *a, **k))[1]
    recorded = {}
    keep = ME.MotionRecorder.export

    def spy(self, *a, **k):
        recorded.update(rb=self.rb[:self.steps].clone(), progress=self.progress[:self.steps].clone())
        return keep(self, *a, **k)
    ME.MotionRecorder.export = spy
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = player.generate_motion(steps)
    finally:
        kernels._launch, ME.MotionRecorder.export = inner, keep
    assert counted.count("pulse_motion_export") == 1, counted                                             # one launch per export
    frames = {k: c["pose_quat_global"].shape[0] for k, c in out.items()}
    assert sum(frames.values()) == steps * envs - out.dropped_frames and all(f >= 2 for f in frames.values()) and all(f < 2 for _, f in out.dropped)
    fps = int(round(1.0 / player.env.task.dt))
    z_dim = before["z"].shape[-1]
    assert all(c["fps"] == fps and c["z"].shape == (frames[k], z_dim) for k, c in out.items())
    # the clips are a motion library
    trees = (syn.SMPL_PARENTS, torch.zeros(len(out), 24, 3))
    lib = MotionLib.from_motion_data(out, trees, device=dev, im_eval=True)
    lib.load_motions(random_sample=False)                                                                 # every clip once, longest first
    assert sorted(lib.curr_motion_keys) == sorted(out)
    rb = recorded["rb"].cpu().double().numpy()
    seg = {k: (e, t0) for k, e, t0 in zip(out.segments["keys"], out.segments["env"].tolist(), out.segments["t0"].tolist())}
    # queried at the exact frame times k / fps: frame k itself, at the bounds tests/test_motion_build_gpu.py holds a queried state to -- lerped
    # quantities (the root position) bit for bit, slerped rotations within 2e-6, as q and not -q
    rb32 = recorded["rb"].cpu()
    for i, key in enumerate(lib.curr_motion_keys):
        e, t0 = seg[key]
        n = frames[key]
        ids = torch.full((n,), i, dtype=torch.int64, device=dev)
        times = (torch.arange(n, dtype=torch.float64) / fps).float().to(dev)
        got = lib.get_motion_state(ids, times)
        rot = rb[t0:t0 + n, e, :, 3:7]
        gap_p = float((got["root_pos"].cpu() - rb32[t0:t0 + n, e, 0, 0:3]).abs().max())
        gap_q = float(np.abs(got["rb_rot"].cpu().double().numpy() - rot).max())
        print(f"{key}: {n} frames, root position gap {gap_p:.3e} (bit for bit asked), rotation gap {gap_q:.3e} (bound 2e-6)")
        assert torch.equal(got["root_pos"].cpu(), rb32[t0:t0 + n, e, 0, 0:3]), key
        assert gap_q <= 2e-6, key
