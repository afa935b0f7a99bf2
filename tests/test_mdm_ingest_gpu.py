"""GPU: pulse_motion_euler_pose and pulse_motion_smooth against the reference's scripts/data_process/convert_data_mdm.py
(tests/golden/mdm_ingest.npz, tools/gen_golden_mdm_ingest.py) and the fp64 restatement (tests/mdm_ingest_model.py), and MotionLib.from_mdm_data /
from_smpl_data(smooth=...) on top of them.

Per output field, over every element, the rule of tests/test_motion_ingest_gpu.py:

    sign(hip) == sign(expected)   and   |hip - expected| <= 4 * err_field

with ``expected`` the reference's fp64 run and ``err_field`` the distance of the reference's OWN fp32 run from it (max over the fixture, stored in
it); a component within the bound of zero must be an exact zero of the expectation, and every quaternion must come out as q, never -q.  What
is a copy (the first 66 columns of pose_aa of the Euler stage's pose, trans_orig of its translation) is compared bit for bit.  The figures
are printed before they are asserted.

Shapes: the four fixture clips (10, 11, 26, 65 frames) packed in one buffer -- 112 frames, 14 workgroups of eight, clip boundaries inside a
workgroup (frame 10) and inside a wave's frame pair (frames 21, 47) -- the same clips shuffled, the 10-frame clip alone (both filters clamp on
both sides at every frame), every clip between neighbour clips of far-away rotations, and the skeleton family's chain / star / SMPL trees at
J = 1, 24 and 32.  Every output and the workspace sit between poison-filled guard rows that must come back untouched.
"""
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
import gen_golden_motion_ingest as GI  # noqa: E402
import mdm_ingest_model as MM  # noqa: E402
import motion_ingest_model as MI  # noqa: E402
import skeleton_cases as SK  # noqa: E402
from pulse_amd import configs, kernels  # noqa: E402
from pulse_amd import synthetic as syn  # noqa: E402
from pulse_amd.env.motion_lib import MotionLib  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 3                                    # poison rows before and after every buffer a kernel writes
POISON = 0x7FC0DEAD                          # a NaN with a payload: any write shows
FIELD_OF = {"euler_pose": "euler_pose", "euler_trans": "euler_trans", "pose_aa": "pose_aa", "trans_orig": "trans_orig", "out_rot": "pose_quat_global",
            "out_trans": "root_trans_offset", "out_pose_quat": "pose_quat"}
WORST = {}                                   # field -> worst |hip - expected| / err seen in this session (printed by the last test)


@pytest.fixture(scope="module")
def fx():
    return GM.load()


@pytest.fixture(scope="module")
def models(fx):
    return [GM.model(c) for c in GM.clips_of(fx)]


def held(got, want, err, name, field=None, zeros=True):
    """sign and value of ``got`` (fp32) against ``want`` (fp64) at 4 x err (module docstring); the figure is printed first.  ``zeros=False``: the
    expectation was computed from fp32 data the device itself produced, where the reference's exact zeros carry that data's rounding residue
    (a hand's global rotation is its wrist's to 6e-8, not to the bit): components inside the bound are then held to the value alone."""
    got = got.astype(np.float64).reshape(want.shape)
    worst = float(np.abs(got - want).max())
    print(f"{name}: max |hip - expected| {worst:.3e} = {worst / err if err else 0.0:.2f} x err ({err:.3e})")
    if field is not None and err:
        WORST[field] = max(WORST.get(field, 0.0), worst / err)
    assert np.isfinite(got).all(), name
    carries = np.abs(want) > 4 * err
    assert not zeros or not SK.settled(want[~carries]).any(), f"{name}: an expected component within the bound of zero is not exactly zero"
    assert np.array_equal(np.sign(got[carries]), np.sign(want[carries])), f"{name}: a sign differs"
    if want.shape[-1] == 4:
        assert ((got * want).sum(-1) > 0).all(), f"{name}: a quaternion came out as -q"
    assert worst <= 4 * err, f"{name}: {worst:.3e} > 4 x {err:.3e}"
    return worst


class Guarded:
    """Poison-filled buffers with GUARD rows before and after the ``total`` rows a kernel may write."""

    def __init__(self, dev, total, shapes):
        self.total = total
        self.full = {k: torch.full((total + 2 * GUARD,) + shape, POISON, dtype=torch.int32, device=dev) for k, shape in shapes.items()}
        self.view = {k: (v if k == "sign_words" else v.view(torch.float32))[GUARD:GUARD + total] for k, v in self.full.items()}

    def check(self, written):
        torch.cuda.synchronize()
        for k, t in self.full.items():
            bits = t.cpu()
            assert (bits[:GUARD] == POISON).all() and (bits[GUARD + self.total:] == POISON).all(), f"{k}: a guard row was written"
            if k in written:
                assert not (bits[GUARD:GUARD + self.total] == POISON).any(), f"{k}: an output element was not written"

    def host(self, k):
        return self.view[k].cpu().numpy()


def smooth_shapes(j):
    return {"out_rot": (j, 4), "out_trans": (3,), "out_pose_quat": (j, 4), "sign_words": ()}


def chain(dev, fx, order, sigma_rot=2.0, sigma_trans=3.0):
    """The three stages on clips ``order`` of the fixture, packed -> (Guarded buffers, frame counts)."""
    clips = [GM.clips_of(fx)[i] for i in order]
    frames = torch.tensor([len(c["thetas"]) for c in clips], dtype=torch.int64)
    total = int(frames.sum())
    theta = torch.from_numpy(np.concatenate([c["thetas"].reshape(-1, 72) for c in clips])).to(dev)
    raw = torch.from_numpy(np.concatenate([c["root_translation"] for c in clips])).to(dev)
    g = Guarded(dev, total, dict({"euler_pose": (72,), "euler_trans": (3,), "ing_rot": (24, 4), "ing_trans": (3,), "pose_aa": (72,), "trans_orig": (3,)},
                                 **smooth_shapes(24)))
    v = g.view
    kernels.motion_euler_pose(v["euler_pose"], v["euler_trans"], src_theta=theta, src_trans=raw, clip_frames=frames)
    kernels.motion_ingest(v["ing_rot"], v["ing_trans"], src_pose=v["euler_pose"], src_trans=v["euler_trans"], clip_src_start=torch.cumsum(frames, 0) - frames,
                          clip_skip=torch.ones_like(frames), clip_frames=frames, parents=syn.SMPL_PARENTS, joint_map=syn.smpl_joint_map(),
                          mirror_map=syn.mirror_body_map(), root_offset=fx["root_offset"].tolist(), out_pose_aa=v["pose_aa"], out_trans_orig=v["trans_orig"])
    kernels.motion_smooth(v["out_rot"], v["out_trans"], in_rot=v["ing_rot"], in_trans=v["ing_trans"], clip_frames=frames, parents=syn.SMPL_PARENTS,
                          sigma_rot=sigma_rot, sigma_trans=sigma_trans, out_pose_quat=v["out_pose_quat"], sign_words=v["sign_words"])
    g.check(set(g.full))
    return g, frames.tolist()


def check_chain(fx, models, g, order, frames, fields=tuple(FIELD_OF), tag=""):
    at = 0
    for i, n in zip(order, frames):
        for k in fields:
            field = FIELD_OF[k]
            got = g.host(k)[at:at + n]
            err = float(fx[f"err_{field}"])
            held(got, fx[f"c{i}_{field}"], err, f"{tag}clip {i} {field} vs golden", field)
            want = models[i]["trans_orig"] if field == "euler_trans" else models[i][field]
            held(got, want, err, f"{tag}clip {i} {field} vs model")
        # the copies: bit for bit
        assert np.array_equal(g.host("pose_aa")[at:at + n, :66].view(np.int32), g.host("euler_pose")[at:at + n, :66].view(np.int32))
        assert not g.host("pose_aa")[at:at + n, 66:].view(np.int32).any()
        assert np.array_equal(g.host("trans_orig")[at:at + n].view(np.int32), g.host("euler_trans")[at:at + n].view(np.int32))
        # the words: the model's raw tests scanned along the clip
        assert np.array_equal(g.host("sign_words")[at:at + n].view(np.uint32), MM.sign_words(models[i]["smooth"]["raw_flip"])[1]), f"{tag}clip {i}: sign words"
        at += n


@pytest.fixture(scope="module")
def packed(dev, fx):
    return chain(dev, fx, [0, 1, 2, 3])


def test_packed_clips_against_golden_and_model(fx, models, packed):
    g, frames = packed
    assert frames == [10, 11, 26, 65] and sum(frames) == 112 == 14 * 8 and frames[0] % 8 != 0 and (frames[0] + frames[1]) % 2 == 1
    check_chain(fx, models, g, [0, 1, 2, 3], frames)


def test_shuffled_clips(dev, fx, models, packed):
    order = [2, 0, 3, 1]
    g, frames = chain(dev, fx, order)
    check_chain(fx, models, g, order, frames, tag="shuffled: ")
    # a clip's values do not depend on where it sits in the buffer
    first = packed[0].host("out_rot")[21:47]
    assert np.array_equal(g.host("out_rot")[:26].view(np.int32), first.view(np.int32))


def test_single_short_clip(dev, fx, models):
    g, frames = chain(dev, fx, [0])
    assert frames == [10] and frames[0] <= 12                 # every frame's taps run past both ends of the clip, rotations (8) and translation (12)
    check_chain(fx, models, g, [0], frames, tag="alone: ")


def _far(n, j, seed):
    """(n, j, 4) constant unit quaternions and (n, 3) translations far from anything a clip holds."""
    q = np.random.default_rng(seed).standard_normal((1, j, 4))
    q = np.repeat(q / np.linalg.norm(q, axis=-1, keepdims=True), n, axis=0)
    return q.astype(np.float32), np.full((n, 3), 50.0 + seed, dtype=np.float32)


def smooth_only(dev, rots, transs, parents, **kw):
    """pulse_motion_smooth on packed clips given as fp32 arrays -> Guarded buffers."""
    j = rots[0].shape[1]
    frames = torch.tensor([len(r) for r in rots], dtype=torch.int64)
    g = Guarded(dev, int(frames.sum()), smooth_shapes(j))
    rot, trans = torch.from_numpy(np.concatenate(rots)).to(dev), torch.from_numpy(np.concatenate(transs)).to(dev)
    kernels.motion_smooth(g.view["out_rot"], g.view["out_trans"], in_rot=rot, in_trans=trans, clip_frames=frames, parents=parents,
                          out_pose_quat=g.view["out_pose_quat"], sign_words=g.view["sign_words"], **kw)
    g.check(set(g.full))
    return g


def check_smooth(fx, g, at, rot32, trans32, parents, name, **kw):
    """Rows [at, at + n) of a smooth_only run against the model on the same fp32 inputs."""
    n = len(rot32)
    res = MM.smooth_clip(rot32, trans32, parents, **kw)
    assert res["gap"].size == 0 or res["gap"].min() > float(fx["gap_floor"])
    assert float(np.linalg.norm(res["filtered"], axis=-1).min()) >= 0.5
    assert len(parents) == 1 or np.abs(res["local_products"][:, 1:, 3]).min() >= float(fx["w_floor"])
    for k, field in (("out_rot", "pose_quat_global"), ("out_pose_quat", "pose_quat"), ("out_trans", "root_trans_offset")):
        held(g.host(k)[at:at + n], res[field], float(fx[f"err_{field}"]), f"{name} {field} vs model")
    assert np.array_equal(g.host("sign_words")[at:at + n].view(np.uint32), MM.sign_words(res["raw_flip"])[1]), f"{name}: sign words"
    return res


@pytest.mark.parametrize("clip", [0, 1, 2, 3])
def test_no_tap_crosses_into_a_neighbour_clip(dev, fx, models, clip):
    """The clip between two clips of constant rotations and translations far from its own: a tap that crossed a boundary would move the result
    by O(0.1) (rotations) and O(10) (translations), a clamp to the buffer instead of the clip likewise."""
    ing = models[clip]["ingest"]
    rot32, trans32 = ing["pose_quat_global"].astype(np.float32), ing["root_trans_offset"].astype(np.float32)
    before, after = _far(20, 24, 1), _far(13, 24, 2)
    g = smooth_only(dev, [before[0], rot32, after[0]], [before[1], trans32, after[1]], syn.SMPL_PARENTS)
    check_smooth(fx, g, 20, rot32, trans32, syn.SMPL_PARENTS, f"clip {clip} between far neighbours")
    # the neighbours themselves: constant clips stay what they were
    for at, (q, t) in ((0, before), (20 + len(rot32), after)):
        held(g.host("out_rot")[at:at + len(q)], q.astype(np.float64), float(fx["err_pose_quat_global"]), "a constant neighbour")
        assert np.abs(g.host("out_trans")[at:at + len(q)] - t).max() <= 4e-6 * 52


def family_inputs(j, frames, seed, parents):
    """``_family_draw`` redrawn (at most 40 times, from seed + 1000, + 2000, ...) until it is quiet in skeleton_cases' sense: every local rotation's
    un-normalised w at least W_FLOOR from zero, no expected component inside (0, ZERO_BAND) -> (rot, trans, redraws)."""
    for attempt in range(40):
        rot, trans = _family_draw(j, frames, seed + 1000 * attempt)
        res = MM.smooth_clip(rot, trans, parents)
        quiet = j == 1 or np.abs(res["local_products"][:, 1:, 3]).min() >= SK.W_FLOOR
        for k in ("pose_quat_global", "pose_quat", "root_trans_offset"):
            a = np.abs(SK.settled(res[k]))
            quiet = quiet and not ((a > 0) & (a < SK.ZERO_BAND)).any()
        if quiet:
            return rot, trans, attempt
    raise AssertionError("the quiet rule rejects nearly everything")


def _family_draw(j, frames, seed):
    """A smooth random rotation path per body with the signs of whole stretches negated (the raw data's sign flips), fp32."""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)[:, None, None]
    axis = rng.standard_normal((1, j, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    half = 0.5 * (rng.uniform(0.3, 2.8, (1, j, 1)) + rng.uniform(-0.12, 0.12, (1, j, 1)) * t + 0.02 * rng.standard_normal((frames, j, 1)))
    q = np.concatenate([np.sin(half) * axis + 0.01 * rng.standard_normal((frames, j, 3)), np.cos(half)], axis=-1)
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    sign = np.where(np.cumsum(rng.random((frames, j)) < 0.12, axis=0) % 2 == 1, -1.0, 1.0)
    sign[:, j // 2] = 1.0 if j > 1 else sign[:, 0]                                      # a body that never flips
    trans = np.cumsum(0.02 * rng.standard_normal((frames, 3)), axis=0) + np.array([0.3, -0.2, 0.9])
    return (q * sign[..., None]).astype(np.float32), trans.astype(np.float32)


@pytest.mark.parametrize("kind,j", [("chain", 1), ("smpl", 24), ("chain", 32), ("star", 32)])
def test_skeleton_family(dev, fx, kind, j):
    parents = SK.parents_of(kind, j)
    clips = [family_inputs(j, n, 100 * j + n, parents) for n in (9, 70, 17)]            # 96 frames; the middle clip crosses a 64-frame step of the scan
    print(f"{kind} J = {j}: redraws {[c[2] for c in clips]}")
    g = smooth_only(dev, [c[0] for c in clips], [c[1] for c in clips], parents)
    at, flips = 0, 0
    for rot32, trans32, _ in clips:
        res = check_smooth(fx, g, at, rot32, trans32, parents, f"{kind} J = {j}, clip at {at}")
        flips += int(res["raw_flip"].sum())
        at += len(rot32)
    assert flips >= 3
    assert j < 32 or (g.host("sign_words").view(np.uint32) >> 31).any()                 # bit 31, the last lane's, is in use


def _flip_bits(x, negated):
    return np.where(negated[..., None], x.view(np.int32) ^ np.int32(-2 ** 31), x.view(np.int32))


def test_sigma_rot_zero_leaves_the_rotations(dev, fx, models):
    g, frames = chain(dev, fx, [0, 1, 2, 3], sigma_rot=0)
    negated = np.concatenate([m["smooth"]["negated"] for m in models])
    assert negated.any() and not negated.all()
    assert np.array_equal(g.host("out_rot").view(np.int32), _flip_bits(g.host("ing_rot"), negated)), "not the input with its sign corrected, bit for bit"
    check_chain(fx, models, g, [0, 1, 2, 3], frames, fields=("out_trans",), tag="sigma_rot 0: ")
    at = 0
    for i, n in enumerate(frames):
        ing = models[i]["ingest"]
        res = MM.smooth_clip(ing["pose_quat_global"], ing["root_trans_offset"], syn.SMPL_PARENTS, sigma_rot=0)
        held(g.host("out_pose_quat")[at:at + n], res["pose_quat"], float(fx["err_pose_quat"]), f"sigma_rot 0: clip {i} pose_quat vs model")
        at += n


def test_sigma_trans_zero_leaves_the_translation(dev, fx, models):
    g, frames = chain(dev, fx, [0, 1, 2, 3], sigma_trans=0)
    assert np.array_equal(g.host("out_trans").view(np.int32), g.host("ing_trans").view(np.int32))
    check_chain(fx, models, g, [0, 1, 2, 3], frames, fields=("out_rot", "out_pose_quat"), tag="sigma_trans 0: ")


def test_wrappers_refuse_by_name(dev):
    rot, trans = torch.zeros(12, 24, 4, device=dev), torch.zeros(12, 3, device=dev)
    frames = torch.tensor([12])
    out = torch.full_like(rot, float("nan"))
    with pytest.raises(ValueError, match=r"radius 13 \(sigma 3.2\)"):
        kernels.motion_smooth(out, torch.empty_like(trans), in_rot=rot, in_trans=trans, clip_frames=frames, parents=syn.SMPL_PARENTS, sigma_rot=3.2)
    with pytest.raises(ValueError, match="out_rot overlaps in_rot"):
        kernels.motion_smooth(rot, torch.empty_like(trans), in_rot=rot, in_trans=trans, clip_frames=frames, parents=syn.SMPL_PARENTS)
    with pytest.raises(ValueError, match="out_trans overlaps in_trans"):
        kernels.motion_smooth(out, trans, in_rot=rot, in_trans=trans, clip_frames=frames, parents=syn.SMPL_PARENTS)
    with pytest.raises(ValueError, match="num_bodies 33"):
        kernels.motion_smooth(torch.zeros(12, 33, 4, device=dev), torch.empty_like(trans), in_rot=torch.zeros(12, 33, 4, device=dev), in_trans=trans,
                              clip_frames=frames, parents=[-1] + list(range(32)))
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------------------------ the library
def trees(slots):
    lt = 0.08 + 0.3 * torch.rand(slots, 24, 3, generator=torch.Generator().manual_seed(3))
    lt[:, 0] = 0.0
    return list(syn.SMPL_PARENTS), lt


def fixture_result(fx):
    clips = GM.clips_of(fx)
    return {"thetas": [c["thetas"] if i % 2 else c["thetas"].reshape(-1, 72).astype(np.float64) for i, c in enumerate(clips)] + [np.zeros((9, 24, 3))],
            "root_translation": [c["root_translation"] if i % 2 else torch.from_numpy(c["root_translation"]) for i, c in enumerate(clips)] + [np.zeros((9, 3))]}


def counting(fn):
    counted, inner = [], kernels._launch
    kernels._launch = lambda name, *a, **k: (counted.append(name), inner(name, *a, **k))[1]
    try:
        return fn(), counted
    finally:
        kernels._launch = inner


def test_from_mdm_data_against_the_fixture_and_round_trip(dev, fx):
    def build():
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            lib = MotionLib.from_mdm_data(fixture_result(fx), trees(6), root_offset=fx["root_offset"].tolist(), device=dev, im_eval=True,
                                          generator=torch.Generator().manual_seed(11))
        return lib, [str(w.message) for w in caught if "from_mdm_data" in str(w.message)]
    (lib, told), counted = counting(build)
    assert [counted.count(n) for n in ("pulse_motion_euler_pose", "pulse_motion_ingest", "pulse_motion_smooth")] == [1, 1, 1], counted
    assert len(told) == 1 and "'4'" not in told[0] and " 4" in told[0] and "fewer than 10" in told[0]
    assert lib._motion_data_keys == ["3", "2", "1", "0"] and (lib._motion_fps == 30).all()           # im_eval: longest first
    md = lib.motion_data()
    assert list(md) == lib._motion_data_keys
    for key, e in md.items():
        i, n = int(key), GM.FRAMES[int(key)]
        assert e["fps"] == 30 and e["gender"] == "neutral" and e["beta"].shape == (10,) and not e["beta"].any()
        assert e["pose_quat_global"].shape == (n, 24, 4) and e["pose_quat"].shape == (n, 24, 4) and e["pose_aa"].shape == (n, 72)
        for k in GM.FIELDS:
            held(e[k], fx[f"c{i}_{k}"], float(fx[f"err_{k}"]), f"motion_data {key} {k}", k)
    again = MotionLib.from_motion_data(md, trees(6), device=dev, im_eval=True, generator=torch.Generator().manual_seed(11))
    assert again._motion_data_keys == lib._motion_data_keys
    for k in ("rot", "trans"):
        assert torch.equal(lib._src[k].view(torch.int32), again._src[k].view(torch.int32)), f"staged {k} differs"
    for k in ("start", "frames", "fps", "has_beta"):
        assert torch.equal(lib._src[k], again._src[k]), k
    assert torch.equal(lib.frames.view(torch.int32), again.frames.view(torch.int32)), "the records differ under im_eval"
    # unsmoothed: the conversion alone
    plain, counted = counting(lambda: MotionLib.from_mdm_data({k: v[:4] for k, v in fixture_result(fx).items()}, trees(4), smooth=None, device=dev,
                                                              root_offset=fx["root_offset"].tolist(), im_eval=True))
    assert "pulse_motion_smooth" not in counted
    assert not torch.equal(plain._src["rot"], lib._src["rot"]) and torch.equal(plain._smpl["pose_aa"].view(torch.int32), lib._smpl["pose_aa"].view(torch.int32))


def test_from_smpl_data_without_smooth_is_what_it_was(dev):
    """smooth=None (the default): the bits of one direct pulse_motion_ingest launch, as before; smooth=True: the same pose_aa / trans_orig, the globals
    of that launch filtered (against the model on those fp32 globals), for a mirrored copy too."""
    gx = GI.load()
    clips = GI.clips_of(gx)
    keep = [0, 1, 2, 4]                                                                            # clip 3 is dropped (2 frames)
    data = {f"c{i}": {"poses": clips[i]["poses"], "trans": clips[i]["trans"], "betas": np.zeros(16), "gender": "male",
                      "mocap_framerate": np.array(clips[i]["framerate"])} for i in keep}
    bounds = {f"c{i}": clips[i]["bound"] for i in keep if clips[i]["bound"]}
    kw = dict(bounds=bounds, root_offset=gx["root_offset"].tolist(), device=dev, mirror=True, generator=torch.Generator().manual_seed(5))
    lib, counted = counting(lambda: MotionLib.from_smpl_data(data, trees(5), **kw))
    assert counted.count("pulse_motion_ingest") == 1 and "pulse_motion_smooth" not in counted and "pulse_motion_euler_pose" not in counted
    dec = [MI.decimate(len(clips[i]["poses"]), clips[i]["framerate"], clips[i]["bound"]) for i in keep for _ in (0, 1)]
    frames = torch.tensor([n for _, n in dec], dtype=torch.int64)
    total = int(frames.sum())
    start = np.cumsum([0] + [len(clips[i]["poses"]) for i in keep])[:-1]
    out = {k: torch.empty((total,) + s, device=dev) for k, s in (("rot", (24, 4)), ("trans", (3,)), ("pose_quat", (24, 4)), ("pose_aa", (72,)), ("trans_orig", (3,)))}
    kernels.motion_ingest(out["rot"], out["trans"], src_pose=torch.from_numpy(np.concatenate([clips[i]["poses"] for i in keep])).to(dev),
                          src_trans=torch.from_numpy(np.concatenate([clips[i]["trans"] for i in keep])).to(dev),
                          clip_src_start=torch.tensor([int(s) for s in start for _ in (0, 1)]), clip_skip=torch.tensor([s for s, _ in dec], dtype=torch.int64),
                          clip_frames=frames, parents=syn.SMPL_PARENTS, joint_map=syn.smpl_joint_map(), mirror_map=syn.mirror_body_map(),
                          clip_mirror=torch.tensor([False, True] * len(keep)), root_offset=gx["root_offset"].tolist(), out_pose_quat=out["pose_quat"],
                          out_pose_aa=out["pose_aa"], out_trans_orig=out["trans_orig"])
    for k in ("rot", "trans"):
        assert torch.equal(lib._src[k].view(torch.int32), out[k].view(torch.int32)), k
    for k in ("pose_quat", "pose_aa", "trans_orig"):
        assert torch.equal(lib._smpl[k].view(torch.int32), out[k].view(torch.int32)), k
    smooth, counted = counting(lambda: MotionLib.from_smpl_data(data, trees(5), smooth={"sigma_rot": 2, "sigma_trans": 3}, **dict(kw, generator=torch.Generator().manual_seed(5))))
    assert counted.count("pulse_motion_ingest") == 1 and counted.count("pulse_motion_smooth") == 1
    for k in ("pose_aa", "trans_orig"):
        assert torch.equal(smooth._smpl[k].view(torch.int32), out[k].view(torch.int32)), k
    fxm = GM.load()
    rot, trans, at, checked = out["rot"].cpu().numpy(), out["trans"].cpu().numpy(), 0, 0
    for n in frames.tolist():
        res = MM.smooth_clip(rot[at:at + n], trans[at:at + n], syn.SMPL_PARENTS)
        # (clip 0 carries rotation vectors of 2 pi - 0.003: two of its steps sit at a gap of 0.007, under the floor the sign test is held at)
        if res["gap"].min() > float(fxm["gap_floor"]) and np.abs(res["local_products"][:, 1:, 3]).min() >= float(fxm["w_floor"]):
            checked += 1
            held(smooth._src["rot"][at:at + n].cpu().numpy(), res["pose_quat_global"], float(fxm["err_pose_quat_global"]), f"smoothed clip at {at} globals", zeros=False)
            held(smooth._smpl["pose_quat"][at:at + n].cpu().numpy(), res["pose_quat"], float(fxm["err_pose_quat"]), f"smoothed clip at {at} pose_quat (its own globals')", zeros=False)
            held(smooth._src["trans"][at:at + n].cpu().numpy(), res["root_trans_offset"], float(fxm["err_root_trans_offset"]), f"smoothed clip at {at} translation", zeros=False)
        at += n
    assert checked >= 6, checked
    with pytest.raises(ValueError, match="smooth requires upright_start=True"):
        MotionLib.from_smpl_data(data, trees(5), smooth=True, upright_start=False, device=dev)


def test_env_on_mdm_data_steps_in_lockstep_with_its_converted_clips(dev):
    """make_env(reference="mdm_data") against an env whose library is built by from_motion_data from the converted clips of the first."""
    from pulse_amd.env.humanoid_im import HumanoidIm, VecTaskPythonWrapper
    from pulse_amd.env.sim import KinematicSim
    n, horizon, seed = 8, 6, 41
    env, _ = configs.make_env(n, horizon, dev, seed=seed, reference="mdm_data")
    mlib = env.task._motion_lib
    assert mlib.reloads and mlib.num_motions() == n and mlib._num_unique_motions == 5 and (mlib._motion_fps == 30).all()
    assert all(e["pose_quat_global"].shape[0] == 196 for e in mlib.motion_data().values())
    g = syn.make_generator(seed + 5, 0)
    _, tr = syn.synthetic_mdm_result(g, 5, jitter=1.0, num_slots=n)                                # the same draws make_env made before the library's own
    bodies, limb = syn.motion_shape_rows(syn.make_generator(7117), n)
    twin_lib = MotionLib.from_motion_data(mlib.motion_data(), tr, gender_betas=bodies, limb_weights=limb, device=dev, generator=g)
    assert twin_lib.curr_motion_keys == mlib.curr_motion_keys
    assert torch.equal(twin_lib.frames.view(torch.int32), mlib.frames.view(torch.int32))
    twin = VecTaskPythonWrapper(HumanoidIm({"env": dict(configs.ENV_IM), "robot": configs.robot_config("smpl")}, KinematicSim(n, horizon + 1, dev, seed=seed, rank=0, humanoid="smpl", dof_limits=None),
                                           twin_lib, device=dev), rl_device=dev)
    a, b = env.reset(), twin.reset()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    gen = torch.Generator().manual_seed(2)
    for _ in range(3):
        act = torch.randn(n, env.task.num_actions, generator=gen).to(dev)
        (oa, ra, da, _), (ob, rb, db, _) = env.step(act), twin.step(act)
        assert torch.isfinite(oa).all() and torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db)
    with pytest.raises(NotImplementedError, match="mdm_data"):
        configs.make_env(n, horizon, dev, reference="mdm_data", humanoid="smplx")


def test_smoothing_lowers_the_angular_velocity_and_the_sign_fix_removes_the_spike(dev):
    """Jittery generated clips: the records' largest angular velocity with smoothing is below the one without; and the sign correction is what keeps
    the filter from producing a spike -- the model's own figures of the filtered globals, with and without quat_correct, say how large."""
    result, tr = syn.synthetic_mdm_result(syn.make_generator(23), 3, frames=[64, 48, 40], jitter=2.0, num_slots=3)
    build = lambda smooth: MotionLib.from_mdm_data(result, tr, smooth=smooth, device=dev, im_eval=True)
    smoothed, rough = build(True), build(None)
    for lib in (smoothed, rough):
        lib.load_motions(random_sample=False)
    top_s, top_r = float(smoothed.gavs.abs().max()), float(rough.gavs.abs().max())

    def speed(q):                                                                                   # rad / s between consecutive frames, per body
        d = np.abs((q[:-1] * q[1:]).sum(-1)) / (np.linalg.norm(q[:-1], axis=-1) * np.linalg.norm(q[1:], axis=-1))
        return 30.0 * 2.0 * np.arccos(np.minimum(d, 1.0))
    with_fix, without_fix, flips = 0.0, 0.0, 0
    for i in range(3):
        res = MM.mdm_clip(result["thetas"][i], result["root_translation"][i], syn.SMPL_PARENTS, syn.smpl_joint_map(), root_offset=tr[1][0, 0].numpy())
        raw = res["ingest"]["pose_quat_global"]
        unfixed = MM.filter_nearest(raw, 2.0)
        with_fix = max(with_fix, float(speed(res["pose_quat_global"]).max()))
        without_fix = max(without_fix, float(speed(unfixed).max()))
        flips += int(res["smooth"]["raw_flip"].sum())
    print(f"max |gavs|: smoothed {top_s:.3f}, unsmoothed {top_r:.3f} rad/s; model: filtered with quat_correct {with_fix:.3f}, without {without_fix:.3f} rad/s; {flips} sign changes")
    assert flips > 0 and top_s < top_r
    assert without_fix > 2.0 * with_fix                       # an uncorrected flip inside the filter window: a spike
    assert top_s <= with_fix * (1 + 1e-3) < without_fix       # the records' filter only averages the per-frame velocities: the library has no spike


def test_worst_ratios_are_reported():
    """Not a check of its own: prints the worst |hip - expected| / err per field over this session's comparisons with the golden (profiles/mdm_ingest.txt)."""
    for k, v in sorted(WORST.items()):
        print(f"worst {k}: {v:.2f} x err")
    assert all(v <= 4.0 for v in WORST.values())
