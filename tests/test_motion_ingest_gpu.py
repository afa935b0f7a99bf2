"""GPU: pulse_motion_ingest against the reference's conversion scripts (tests/golden/motion_ingest.npz, tools/gen_golden_motion_ingest.py) and the
fp64 restatement (tests/motion_ingest_model.py), and MotionLib.from_smpl_data on top of it.

Per output field, over every element

    sign(hip) == sign(expected)   and   |hip - expected| <= 4 * err_field

with ``expected`` the reference's fp64 run and ``err_field`` the distance of the reference's OWN fp32 run from it (max over the fixture, stored in
it): the tolerance is made of the reference's error alone, with the margin tests/test_motion_build_gpu.py uses against the same kind of
yardstick.  pose_aa and trans_orig are copies: err is 0 and they must be exact.  The sign is compared on every element larger than the bound
(a component within 4 x err of zero has no sign the bound lets fp32 keep: the hands' local rotations are exactly (0, 0, 0, 1) in the fp64 run
and carry a rounding residue of +-6e-8 in any fp32 evaluation, the reference's own included -- and the test asserts that exact zeros are the ONLY
expected components that small), and every quaternion as a whole must be q, not -q.  The figures are printed before they are asserted.

The kernel runs on clips of 10, 11, 37 and 2 (cut by ``bound``) converted frames: 60 output frames, 7.5 workgroups of eight frames, the first
clip boundary inside workgroup 1.  Every output sits between poison-filled guard rows that must come back untouched.
``upright_start=False`` has no runnable counterpart in the reference: it is held to the model alone, at the same bounds.

Library: from_smpl_data -> motion_data() -> from_motion_data stages the same bits (and builds the same records under im_eval); the records'
grs / lrs / root gts against the golden at 4 x err, and EVERY record field against a library built from the golden's converted dict (positions
and velocities at bounds derived from those input gaps, stated in the test); an env built with reference="smpl_data" resets and steps; one launch per ingest."""
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

import gen_golden_motion_ingest as GI  # noqa: E402
import motion_ingest_model as MI  # noqa: E402
from pulse_amd import configs, kernels  # noqa: E402
from pulse_amd import synthetic as syn  # noqa: E402
from pulse_amd.env.motion_lib import MotionLib  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 3                                    # poison rows before and after every output
POISON = 0x7FC0DEAD                          # a NaN with a payload: any write shows
OUT = {"out_rot": (24, 4), "out_trans": (3,), "out_pose_quat": (24, 4), "out_pose_aa": (72,), "out_trans_orig": (3,)}
FIELD_OF = {"out_rot": "pose_quat_global", "out_trans": "root_trans_offset", "out_pose_quat": "pose_quat", "out_pose_aa": "pose_aa",
            "out_trans_orig": "trans_orig"}


@pytest.fixture(scope="module")
def fx():
    return GI.load()


def model(fx, clip, **kw):
    return MI.ingest_clip(clip["poses"], clip["trans"], clip["framerate"], syn.SMPL_PARENTS, syn.smpl_joint_map(), bound=clip["bound"],
                          root_offset=fx["root_offset"], mirror_map=syn.mirror_body_map(), **kw)


def ingest(dev, fx, which, mirror=None, upright_start=True):
    """The kernel on clips ``which`` of the fixture (``mirror``: per clip) -> (outputs with their guard rows, clip frame counts)."""
    clips = GI.clips_of(fx)
    start, at = [], 0
    for c in clips:                                            # every raw clip is staged, whichever are converted
        start.append(at)
        at += len(c["poses"])
    pose = torch.from_numpy(np.concatenate([c["poses"] for c in clips])).to(dev)
    trans = torch.from_numpy(np.concatenate([c["trans"] for c in clips])).to(dev)
    dec = [MI.decimate(len(clips[i]["poses"]), clips[i]["framerate"], clips[i]["bound"]) for i in which]
    frames = torch.tensor([n for _, n in dec], dtype=torch.int64)
    total = int(frames.sum())
    full = {k: torch.full((total + 2 * GUARD,) + shape, POISON, dtype=torch.int32, device=dev).view(torch.float32) for k, shape in OUT.items()}
    view = {k: v[GUARD:GUARD + total] for k, v in full.items()}
    kernels.motion_ingest(view["out_rot"], view["out_trans"], src_pose=pose, src_trans=trans, clip_src_start=torch.tensor([start[i] for i in which]),
                          clip_skip=torch.tensor([s for s, _ in dec], dtype=torch.int64), clip_frames=frames, parents=syn.SMPL_PARENTS,
                          joint_map=syn.smpl_joint_map(), mirror_map=syn.mirror_body_map(), clip_mirror=None if mirror is None else torch.tensor(mirror),
                          upright_start=upright_start, root_offset=fx["root_offset"].tolist(), out_pose_quat=view["out_pose_quat"],
                          out_pose_aa=view["out_pose_aa"], out_trans_orig=view["out_trans_orig"])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in full.items()}, frames.tolist()


def held(got, want, err, name):
    """sign and value of ``got`` (fp32) against ``want`` (fp64) at 4 x err (module docstring); the figure is printed first."""
    got = got.astype(np.float64).reshape(want.shape)
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


@pytest.fixture(scope="module")
def plain(dev, fx):
    return ingest(dev, fx, [0, 1, 2, 3])


def test_kernel_against_golden_and_model(fx, plain):
    full, frames = plain
    assert frames == [10, 11, 37, 2] and sum(frames) % 8 != 0 and frames[0] % 8 != 0
    at = GUARD
    for i, n in enumerate(frames):
        res = model(fx, GI.clips_of(fx)[i])
        for k, field in FIELD_OF.items():
            got = full[k][at:at + n].numpy()
            held(got, fx[f"c{i}_{field}"], float(fx[f"err_{field}"]), f"clip {i} {field} vs golden")
            held(got, res[field], float(fx[f"err_{field}"]), f"clip {i} {field} vs model")
        at += n


def test_guard_rows_stay_poisoned(plain):
    full, frames = plain
    total = sum(frames)
    for k, t in full.items():
        bits = t.view(torch.int32)
        assert (bits[:GUARD] == POISON).all() and (bits[GUARD + total:] == POISON).all(), f"{k}: a guard row was written"
        assert not (bits[GUARD:GUARD + total] == POISON).any(), f"{k}: an output element was not written"


def test_mirrored_copies(dev, fx, plain):
    """Every clip followed by its mirrored copy (the ``double`` loop of convert_amass_isaac.py:90-126), clip boundaries off the workgroup grid."""
    which, mirror = [0, 0, 1, 1, 3, 3], [False, True] * 3
    full, frames = ingest(dev, fx, which, mirror)
    at = GUARD
    for i, m, n in zip(which, mirror, frames):
        res = model(fx, GI.clips_of(fx)[i], mirror=m)
        pre = "mirror_" if m else ""
        for k, field in FIELD_OF.items():
            got = full[k][at:at + n].numpy()
            golden = f"c{i}_{pre}{field}" if field in GI.MIRROR_FIELDS else f"c{i}_{field}"      # the copy keeps pose_quat / pose_aa / trans_orig
            held(got, fx[golden], float(fx[f"err_{field}"]), f"clip {i}{' mirrored' if m else ''} {field} vs golden")
            held(got, res[field], float(fx[f"err_{field}"]), f"clip {i}{' mirrored' if m else ''} {field} vs model")
        if m:
            for k in ("out_pose_quat", "out_pose_aa", "out_trans_orig"):
                assert torch.equal(full[k][at:at + n].view(torch.int32), full[k][at - n:at].view(torch.int32)), k
        at += n
    # the unmirrored clips are the bits of the plain run
    assert torch.equal(full["out_rot"][GUARD:GUARD + 10].view(torch.int32), plain[0]["out_rot"][GUARD:GUARD + 10].view(torch.int32))


def test_without_upright_start_against_the_model(dev, fx):
    full, frames = ingest(dev, fx, [0, 2], upright_start=False)
    at = GUARD
    for i, n in zip([0, 2], frames):
        res = model(fx, GI.clips_of(fx)[i], upright_start=False)
        for k, field in FIELD_OF.items():
            held(full[k][at:at + n].numpy(), res[field], float(fx[f"err_{field}"]), f"clip {i} {field}, no upright factor, vs model")
        at += n


def test_33_bodies_are_refused_by_name(dev):
    parents = [-1] + list(range(32))
    rot, trans = torch.full((4, 33, 4), float("nan"), device=dev), torch.full((4, 3), float("nan"), device=dev)
    with pytest.raises(ValueError, match="num_bodies 33"):
        kernels.motion_ingest(rot, trans, src_pose=torch.zeros(4, 72, device=dev), src_trans=torch.zeros(4, 3, device=dev),
                              clip_src_start=torch.tensor([0]), clip_skip=torch.tensor([1]), clip_frames=torch.tensor([4]), parents=parents,
                              joint_map=list(range(24)) + [0] * 9)
    torch.cuda.synchronize()
    assert torch.isnan(rot).all() and torch.isnan(trans).all()
    with pytest.raises(TypeError, match="CUDA tensor"):
        kernels.motion_ingest(rot[:, :24].contiguous(), trans, src_pose=torch.zeros(4, 72), src_trans=torch.zeros(4, 3, device=dev),
                              clip_src_start=torch.tensor([0]), clip_skip=torch.tensor([1]), clip_frames=torch.tensor([4]), parents=syn.SMPL_PARENTS,
                              joint_map=syn.smpl_joint_map())


# ------------------------------------------------------------------------------------------------------------------ the library
def raw_data(fx):
    """The fixture's clips as a data set ships them: both spellings of the keys, fp32 and fp64, numpy and torch."""
    data = {}
    for i, c in enumerate(GI.clips_of(fx)):
        e = {"trans": c["trans"] if i % 2 else torch.from_numpy(c["trans"]).double(), "gender": "male", "mocap_framerate": np.array(c["framerate"])}
        e["poses" if i % 2 else "pose_aa"] = c["poses"].astype(np.float64) if i % 2 else c["poses"]
        e["betas" if i % 2 else "beta"] = np.ones(16 if i % 2 else 10)
        data[f"c{i}"] = e
    return data, {f"c{i}": c["bound"] for i, c in enumerate(GI.clips_of(fx)) if c["bound"]}


def trees(slots):
    lt = 0.08 + 0.3 * torch.rand(slots, 24, 3, generator=torch.Generator().manual_seed(3))
    lt[:, 0] = 0.0
    return list(syn.SMPL_PARENTS), lt


def build_lib(dev, fx, **kw):
    data, bounds = raw_data(fx)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        lib = MotionLib.from_smpl_data(data, trees(kw.pop("slots", 6)), bounds=bounds, root_offset=fx["root_offset"].tolist(), device=dev, **kw)
    return lib, [str(w.message) for w in caught if "from_smpl_data" in str(w.message)]


@pytest.mark.parametrize("mirror", [False, True])
def test_round_trip_through_motion_data(dev, fx, mirror):
    counted = []
    inner = kernels._launch
    kernels._launch = lambda name, *a, **k: (counted.append(name), inner(name, *a, **k))[1]
    try:
        lib, told = build_lib(dev, fx, mirror=mirror, im_eval=True, generator=torch.Generator().manual_seed(11))
    finally:
        kernels._launch = inner
    assert counted.count("pulse_motion_ingest") == 1, counted                                       # one launch per ingest
    assert len(told) == 1 and "c3" in told[0] and "fewer than 10" in told[0]                         # the user is told which clip went
    keys = ["c2", "c4", "c1", "c0"]                                                                  # im_eval: longest first (37, 13, 11, 10)
    assert lib._motion_data_keys == ([k + s for k in keys for s in ("", "_1")] if mirror else keys)
    md = lib.motion_data()
    assert list(md) == lib._motion_data_keys
    for key, e in md.items():
        i = int(key[1])
        n = {0: 10, 1: 11, 2: 37, 4: 13}[i]
        assert e["fps"] == 30 and e["gender"] == "neutral" and e["beta"].shape == ((16,) if i % 2 else (10,)) and not e["beta"].any()
        assert e["pose_quat_global"].shape == (n, 24, 4) and e["pose_quat"].shape == (n, 24, 4) and e["pose_aa"].shape == (n, 72)
        assert e["root_trans_offset"].shape == (n, 3) and e["trans_orig"].shape == (n, 3)
        pre = "mirror_" if key.endswith("_1") else ""
        held(e["pose_quat_global"], fx[f"c{i}_{pre}pose_quat_global"], float(fx["err_pose_quat_global"]), f"{key} pose_quat_global")
        held(e["root_trans_offset"], fx[f"c{i}_{pre}root_trans_offset"], float(fx["err_root_trans_offset"]), f"{key} root_trans_offset")
        for k in ("pose_quat", "pose_aa", "trans_orig"):                                             # a mirrored clip carries the unmirrored ones
            held(e[k], fx[f"c{i}_{k}"], float(fx[f"err_{k}"]), f"{key} {k}")
    again = MotionLib.from_motion_data(md, trees(6), device=dev, im_eval=True, generator=torch.Generator().manual_seed(11))
    assert again._motion_data_keys == lib._motion_data_keys
    for k in ("rot", "trans"):
        assert torch.equal(lib._src[k].view(torch.int32), again._src[k].view(torch.int32)), f"staged {k} differs"
    for k in ("start", "frames", "fps", "has_beta"):
        assert torch.equal(lib._src[k], again._src[k]), k
    assert lib.curr_motion_keys == again.curr_motion_keys
    assert torch.equal(lib.frames.view(torch.int32), again.frames.view(torch.int32)), "the records differ under im_eval"
    with pytest.raises(ValueError, match="from_smpl_data"):
        again.motion_data()


def _vec_norm_of_steps(q, first_conj):
    """|vector part| = sin(angle / 2) of the frame-to-frame rotation of every body, fp64: conj(q[t]) q[t+1] (``first_conj``) or q[t+1] conj(q[t]);
    the last frame repeats the step before it (it has none of its own)."""
    c = np.array([-1.0, -1.0, -1.0, 1.0])
    d = MI.quat_mul(q[:-1] * c, q[1:]) if first_conj else MI.quat_mul(q[1:], q[:-1] * c)
    sh = np.linalg.norm(d[..., :3], axis=-1) / np.linalg.norm(d, axis=-1)
    return np.concatenate([sh, sh[-1:]])


def _rotvec_gap(sh, eps):
    """How far two fp32 evaluations of  axis * angle  of a unit quaternion may lie apart when each has its components within ``eps`` of the
    true ones and sin(angle / 2) = ``sh``.  The angle comes from w alone (acos(2 w^2 - 1) in poselib, 2 acos(w) in torch_utils): an error
    eps in w moves it by 2 eps / sh, and never by more than sqrt(8 eps) (at sh -> 0, where angle^2 ~ 8 (1 - w)); the axis v / |v| times
    the angle moves by at most pi eps (angle / |v| <= pi).  Twice that: each evaluation is off on its own."""
    with np.errstate(divide="ignore"):
        return 2.0 * (np.minimum(2.0 * eps / sh, np.sqrt(8.0 * eps)) + np.pi * eps)


def test_records_against_the_golden_converted_data(dev, fx):
    """Every field of the records, under im_eval (no heading draw), against a library built from the golden's converted dict by the same kernels
    with the same skeletons -- and grs / lrs / root gts, which ARE pose_quat_global / pose_quat / root_trans_offset, against the golden itself.

    grs, lrs and gts[:, 0] are held to the issue's 4 x err.  The other fields are functions of them, and the literal 4 x err cannot hold for a
    derivative: the bound is the first-order propagation of those input gaps (dq = 4 err_pose_quat_global, dl = 4 err_pose_quat,
    dt = 4 err_root_trans_offset, per component; a quaternion's 2-norm gap is at most twice its component gap) plus the fp32 rounding of the
    evaluation itself (u = 2^-23):
      gts   a body at depth k hangs on k rotated bone offsets of length <= L.  R of depth k is k quat_mul_norm by lrs on the root's grs:
            |dR|_2 <= 2 dq + k (2 dl + 2 err_pose_quat); rotating v moves it by <= 2 |dR|_2 |v|.
            gap <= dt + sum_{k < D} 2 L (2 dq + k (2 dl + 2 err_pose_quat)) + 4 (D + 1) u max|gts|
      gvs   np.gradient / dt (a first difference at a clip's ends: two positions, times fps), a filter of positive weights that sum to 1:
            gap <= 2 fps gap(gts) + 4 u max|gvs|
      gavs  axis * angle * fps of q[t+1] conj(q[t]) (2-norm gap of the product eps_g = 4 dq + 4 u), per frame and body by _rotvec_gap, the
            filter taking at most the largest value of its 17-frame window inside the clip; + 4 u max|gavs|
      dvs   the same of conj(l[t]) l[t+1] with eps_l = 4 dl + 4 u, no filter; + 4 u max|dvs|
    A wrong fps label, a filter fed across a clip boundary or a wrong root offset moves these fields by 1e-2 .. 1 and more."""
    lib, _ = build_lib(dev, fx, slots=4, im_eval=True)
    lib.load_motions(random_sample=False)
    gold = {f"c{i}": {"pose_quat_global": fx[f"c{i}_pose_quat_global"], "root_trans_offset": fx[f"c{i}_root_trans_offset"], "fps": 30, "beta": np.zeros(16)}
            for i in (0, 1, 2, 4)}
    ref = MotionLib.from_motion_data(gold, trees(4), device=dev, im_eval=True)
    ref.load_motions(random_sample=False)
    assert lib.curr_motion_keys == ref.curr_motion_keys == ["c2", "c4", "c1", "c0"]
    assert torch.equal(lib._motion_num_frames, ref._motion_num_frames) and torch.equal(lib._motion_lengths, ref._motion_lengths)
    assert torch.equal(lib._motion_fps, ref._motion_fps) and torch.equal(lib.length_starts, ref.length_starts)
    want = {k: np.concatenate([fx[f"{c}_{k}"] for c in lib.curr_motion_keys]) for k in ("pose_quat_global", "pose_quat", "root_trans_offset")}
    err = {k: float(fx[f"err_{k}"]) for k in want}
    mine = {k: getattr(lib, k).cpu().numpy().astype(np.float64) for k in MotionLib.FIELDS}
    theirs = {k: getattr(ref, k).cpu().numpy().astype(np.float64) for k in MotionLib.FIELDS}
    for name, got, field in (("grs", mine["grs"], "pose_quat_global"), ("lrs", mine["lrs"], "pose_quat"), ("gts[:, 0]", mine["gts"][:, 0], "root_trans_offset")):
        held(got.astype(np.float32), want[field], err[field], f"records {name} vs golden {field}")
    # the derived bounds (docstring)
    dq, dl, dt, u, fps = 4 * err["pose_quat_global"], 4 * err["pose_quat"], 4 * err["root_trans_offset"], 2.0 ** -23, 30.0
    parents, lt = trees(4)
    depth = [0] * 24
    for b in range(1, 24):
        depth[b] = depth[parents[b]] + 1
    D, L = max(depth), float(lt.norm(dim=-1).max())
    big = {k: float(np.abs(theirs[k]).max()) for k in theirs}
    gts_gap = dt + sum(2 * L * (2 * dq + k * (2 * dl + 2 * err["pose_quat"])) for k in range(D)) + 4 * (D + 1) * u * big["gts"]
    bound = {"grs": dq, "lrs": dl, "gts": gts_gap, "gvs": 2 * fps * gts_gap + 4 * u * big["gvs"]}
    gavs_b, dvs_b = [], []
    for c in lib.curr_motion_keys:
        raw = fps * _rotvec_gap(_vec_norm_of_steps(fx[f"{c}_pose_quat_global"], False), 4 * dq + 4 * u)
        n = raw.shape[0]
        gavs_b.append(np.stack([raw[max(0, t - 8):min(n, t + 9)].max(0) for t in range(n)]))
        dvs_b.append(fps * _rotvec_gap(_vec_norm_of_steps(fx[f"{c}_pose_quat"][:, 1:], True), 4 * dl + 4 * u))
    bound["gavs"] = np.concatenate(gavs_b)[..., None] + 4 * u * big["gavs"]
    bound["dvs"] = np.concatenate(dvs_b)[..., None] + 4 * u * big["dvs"]
    worst = {}
    for k in MotionLib.FIELDS:
        gap = np.abs(mine[k] - theirs[k])
        worst[k] = float((gap / bound[k]).max())
        print(f"records {k} vs the golden-built library: max gap {gap.max():.3e}, largest gap / bound {worst[k]:.3f} "
              f"(bound {float(np.min(bound[k])):.3e} .. {float(np.max(bound[k])):.3e}; max |{k}| {big[k]:.3f})")
    assert float(np.abs(mine["gts"][:, 0] - theirs["gts"][:, 0]).max()) <= dt
    for k in MotionLib.FIELDS:
        assert np.isfinite(mine[k]).all() and worst[k] <= 1.0, (k, worst[k])


def test_env_on_raw_smpl_data_resets_and_steps(dev):
    n = 8
    env, _ = configs.make_env(n, 6, dev, seed=41, reference="smpl_data")
    task = env.task
    mlib = task._motion_lib
    assert mlib.reloads and mlib.num_motions() == n and mlib._num_unique_motions == 5 and (mlib._motion_fps == 30).all()
    assert set(mlib.motion_data()) == set(mlib._motion_data_keys)
    obs = env.reset()
    assert torch.isfinite(obs).all()
    g = torch.Generator().manual_seed(2)
    for _ in range(3):
        obs, rew, done, info = env.step(torch.randn(n, task.num_actions, generator=g).to(dev))
        assert torch.isfinite(obs).all() and torch.isfinite(rew).all()
    obs = env.reset(torch.arange(n, device=dev))
    assert torch.isfinite(obs).all()
    task.resample_motions()
    assert torch.isfinite(env.reset()).all()
    with pytest.raises(NotImplementedError, match="smpl_data"):
        configs.make_env(n, 6, dev, reference="smpl_data", humanoid="smplx")
