"""GPU: pulse_motion_ingest, pulse_motion_export and pulse_keypoint_push on skeletons other than SMPL's (tests/skeleton_cases.py: chains of depth 31,
stars, random trees, a deep level beside low-numbered parents; 1 .. 32 bodies; joint and mirror maps that are not their own inverse) against the
fp64 restatements (tests/motion_ingest_model.py, motion_export_model.py, keypoint_stream_model.py), which tests/test_half_wave_shapes_cpu.py holds
to scipy over the same family.

The rule of the sibling tests, unchanged (their ``held`` is imported): the sign matches on every component above the bound, the expected components
below it are exact zeros, every quaternion comes out as q and not -q, and

    |hip - fp64 model| <= 4 x err_field

with err_field from profiles/half_wave_shapes.txt: max |model(float32) - model(float64)| over this family, floored at the golden fixture's figure
for the field (recomputed by the CPU test).  Copies are compared bit for bit.  Every output and every state buffer sits between poison rows
(0x7FC0DEAD) that must come back untouched, and every element inside must have been written.  Every figure is printed before it is asserted;
the worst ratio per kernel and field is printed when the module is done (copied into the profile)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import motion_export_model as MX  # noqa: E402
import skeleton_cases as SC  # noqa: E402
from pulse_amd import kernels  # noqa: E402
from test_keypoint_stream_gpu import held as held_stream  # noqa: E402
from test_motion_export_gpu import held  # noqa: E402  (the ingest test's, with np.asarray in front)

pytestmark = pytest.mark.gpu
GUARD = 3                                    # poison rows before and after every buffer
POISON = 0x7FC0DEAD                          # a NaN with a payload: any write shows
ERR = {k: v[0] for k, v in SC.stored_yardsticks().items()}
WORST = {}
INGEST_OUT = {"out_rot": "pose_quat_global", "out_trans": "root_trans_offset", "out_pose_quat": "pose_quat", "out_pose_aa": "pose_aa",
              "out_trans_orig": "trans_orig"}
EXPORT_OUT = dict(INGEST_OUT, out_body_quat="body_quat", out_dof_pos="dof_pos")
TOTALS_INGEST, TOTALS_EXPORT = (1, 7, 8, 9, SC.FRAMES), (1, 8, 9, SC.FRAMES)


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    for (kernel, field), r in sorted(WORST.items()):
        print(f"\nworst {kernel} {field}: {r:.2f} x err ({ERR[kernel, field]:.3e})", end="")
    print()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def hold(kernel, field, got, want, name):
    """One field of one launch against the fp64 model: a copy bit for bit, anything else by the siblings' rule at 4 x err_field."""
    if field in SC.COPIES[kernel]:
        assert np.array_equal(bits(got).reshape(want.shape), bits(want)), f"{name}: a copy differs"
        return
    if not want.size:
        return
    err = ERR[kernel, field]
    worst = (held_stream if kernel == "keypoint" else held)(got, SC.settled(want), err, name)
    WORST[kernel, field] = max(WORST.get((kernel, field), 0.0), worst / err)


class Guarded:
    """Device buffers, each the middle of a poison-filled allocation with GUARD rows before and after."""

    def __init__(self, dev, rows, shapes, dtypes=None):
        self.rows, self.full, self.view = rows, {}, {}
        for k, s in shapes.items():
            full = torch.full((rows + 2 * GUARD,) + tuple(s), POISON, dtype=torch.int32, device=dev)
            self.full[k] = full
            self.view[k] = full[GUARD:GUARD + rows] if (dtypes or {}).get(k) == torch.int32 else full.view(torch.float32)[GUARD:GUARD + rows]

    def check(self, what, written=True):
        torch.cuda.synchronize()
        for k, full in self.full.items():
            b = full.cpu()
            assert (b[:GUARD] == POISON).all() and (b[GUARD + self.rows:] == POISON).all(), f"{what} {k}: a guard row was written"
            if written:
                assert not (b[GUARD:GUARD + self.rows] == POISON).any(), f"{what} {k}: an element was not written"

    def numpy(self):
        return {k: v.cpu().numpy() for k, v in self.view.items()}


# ------------------------------------------------------------------------------------------------------------------ ingest
def run_ingest(dev, c, poses, trans, clips, upright=True, outputs=tuple(INGEST_OUT)):
    """The kernel on ``clips`` [(src_start, skip, frames, mirror)] of the staged ``poses`` / ``trans`` -> {output: array} (guards checked)."""
    j, total = c["j"], sum(f for _, _, f, _ in clips)
    shapes = {"out_rot": (j, 4), "out_trans": (3,), "out_pose_quat": (j, 4), "out_pose_aa": (72,), "out_trans_orig": (3,)}
    g = Guarded(dev, total, {k: shapes[k] for k in outputs})
    table = lambda i: torch.tensor([cl[i] for cl in clips], dtype=torch.int64)
    mirror = torch.tensor([cl[3] for cl in clips]) if any(cl[3] for cl in clips) else None
    kernels.motion_ingest(g.view["out_rot"], g.view["out_trans"], src_pose=torch.from_numpy(poses).to(dev), src_trans=torch.from_numpy(trans).to(dev),
                          clip_src_start=table(0), clip_skip=table(1), clip_frames=table(2), parents=c["parents"], joint_map=c["ingest_map"],
                          mirror_map=c["mirror_map"], clip_mirror=mirror, upright_start=upright, root_offset=SC.ROOT_OFFSET.tolist(),
                          **{k: v for k, v in g.view.items() if k not in ("out_rot", "out_trans")})
    g.check(f"ingest {c['kind']} J = {j}")
    return g.numpy()


def ingest_rows(clips):
    return [s + i * k for s, k, f, _ in clips for i in range(f)], [m for _, _, f, m in clips for _ in range(f)]


def ingest_against_model(dev, c, poses, trans, clips, upright, what):
    got = run_ingest(dev, c, poses, trans, clips, upright)
    rows, mirrored = ingest_rows(clips)
    plain, flipped = SC.ingest_model(c, poses, trans, upright_start=upright), SC.ingest_model(c, poses, trans, upright_start=upright, mirror=True)
    for k, field in INGEST_OUT.items():
        want = np.stack([(flipped if m else plain)[field][r] for r, m in zip(rows, mirrored)])
        hold("ingest", field, got[k], want, f"ingest {c['kind']} J = {c['j']} upright {upright} {what} {field}")
    return got


@pytest.mark.parametrize("upright", [True, False])
@pytest.mark.parametrize("kind", SC.TREES)
def test_ingest_every_tree_and_body_count(dev, kind, upright):
    for c in SC.cases("ingest", kind):
        poses, trans, _ = SC.ingest_inputs(c)
        for total in TOTALS_INGEST:
            plain = ingest_against_model(dev, c, poses, trans, [(0, 1, total, False)], upright, f"{total} frames")
        # every frame once plain and once mirrored, in one launch: 38 frames, the boundary inside workgroup 2
        both = ingest_against_model(dev, c, poses, trans, [(0, 1, SC.FRAMES, False), (0, 1, SC.FRAMES, True)], upright, "plain + mirrored")
        for k in INGEST_OUT:
            assert np.array_equal(bits(both[k][:SC.FRAMES]), bits(plain[k])), f"{k}: the unmirrored clip lost the bits of the plain run"
        for k in ("out_pose_quat", "out_pose_aa", "out_trans_orig"):                     # the mirrored copy keeps these
            assert np.array_equal(bits(both[k][SC.FRAMES:]), bits(plain[k])), k


def test_ingest_with_the_required_outputs_only(dev):
    c = SC.case("ingest", "random", 31)
    poses, trans, _ = SC.ingest_inputs(c)
    clips = [(0, 1, SC.FRAMES, False)]
    full, two = run_ingest(dev, c, poses, trans, clips), run_ingest(dev, c, poses, trans, clips, outputs=("out_rot", "out_trans"))
    assert sorted(two) == ["out_rot", "out_trans"]
    for k in two:
        assert np.array_equal(bits(two[k]), bits(full[k])), k


@pytest.mark.parametrize("kind,j", [("chain", 1), ("late_low", 6), ("random", 31), ("chain", 32)])
def test_ingest_clip_tables(dev, kind, j):
    c = SC.case("ingest", kind, j)
    poses, trans, _ = SC.ingest_inputs(c)
    # every output frame a clip of its own, read from a shuffled staged frame: a wrong clip looked up for a frame reads another one
    order = np.random.default_rng(j).permutation(SC.FRAMES)
    assert not np.array_equal(order, np.arange(SC.FRAMES))
    ingest_against_model(dev, c, poses, trans, [(int(s), 1, 1, False) for s in order], True, "19 one-frame clips")
    # decimated clips (skip 2 and 4), the second one's last read exactly the last staged frame
    clips = [(0, 2, 5, False), (2, 4, 5, False)]
    assert clips[1][0] + (clips[1][2] - 1) * clips[1][1] == SC.FRAMES - 1 == len(poses) - 1
    ingest_against_model(dev, c, poses, trans, clips, True, "skips 2 and 4")
    # three staged clips [0, 5), [5, 12), [12, 19) converted in another order, the last one twice
    clips = [(12, 1, 7, False), (0, 1, 5, False), (12, 1, 7, True), (5, 1, 7, False)]
    got = ingest_against_model(dev, c, poses, trans, clips, True, "out of staging order")
    assert np.array_equal(bits(got["out_pose_quat"][:7]), bits(got["out_pose_quat"][12:19]))


# ------------------------------------------------------------------------------------------------------------------ export
def strided(dev, a, pad):
    """``a`` as a view into a larger NaN-filled device buffer: ``pad`` = per dimension (before, after)."""
    big = torch.full([s + p + q for s, (p, q) in zip(a.shape, pad)], float("nan"), device=dev)
    view = big[tuple(slice(p, p + s) for s, (p, _) in zip(a.shape, pad))]
    view.copy_(torch.from_numpy(a))
    assert not view.numel() or not view.is_contiguous()
    return view


def run_export(dev, c, rb, dof, segs, upright=True, outputs=tuple(EXPORT_OUT), use_dof=True):
    j, total = c["j"], sum(s[2] for s in segs)
    shapes = {"out_rot": (j, 4), "out_trans": (3,), "out_pose_quat": (j, 4), "out_pose_aa": (3 * j,), "out_trans_orig": (3,), "out_body_quat": (j, 4),
              "out_dof_pos": (3 * (j - 1),)}
    g = Guarded(dev, total, {k: shapes[k] for k in outputs})
    table = lambda i: torch.tensor([s[i] for s in segs], dtype=torch.int64)
    kernels.motion_export(g.view["out_rot"], g.view["out_trans"], rb=strided(dev, rb, [(1, 1), (2, 1), (1, 1), (0, 3)]),
                          dof_pos=strided(dev, dof, [(1, 0), (1, 1), (0, 3)]) if use_dof else None, seg_env=table(0), seg_t0=table(1), seg_frames=table(2),
                          parents=c["parents"], joint_map=c["joint_map"], upright_start=upright, root_offset=SC.ROOT_OFFSET.tolist(),
                          **{k: v for k, v in g.view.items() if k not in ("out_rot", "out_trans")})
    g.check(f"export {c['kind']} J = {j}")
    return g.numpy()


def export_against_model(dev, c, rb, dof, segs, upright, what):
    got = run_export(dev, c, rb, dof, segs, upright)
    res = SC.export_model(c, *MX.gather(rb, dof, segs), upright_start=upright)
    for k, field in EXPORT_OUT.items():
        hold("export", field, got[k], res[field], f"export {c['kind']} J = {c['j']} upright {upright} {what} {field}")
    return got, res


@pytest.mark.parametrize("upright", [True, False])
@pytest.mark.parametrize("kind", SC.TREES)
def test_export_every_tree_and_body_count(dev, kind, upright):
    for c in SC.cases("export", kind):
        rb, dof, _ = SC.export_inputs(c)
        j = c["j"]
        segs = SC.one_frame_segments(c)
        assert len(segs) == SC.FRAMES and all(s[2] == 1 for s in segs) and segs != sorted(segs)
        for total in TOTALS_EXPORT:
            got, res = export_against_model(dev, c, rb, dof, segs[:total], upright, f"{total} one-frame segments")
        if j >= 3:                                               # the test can tell joint_map from its inverse: the model with the inverse differs by more than the bound
            other = MX.export_frames(*MX.gather(rb, dof, segs), c["parents"], SC.inverse(c["joint_map"]), upright_start=upright, root_offset=SC.ROOT_OFFSET)
            assert float(np.abs(other["pose_aa"] - res["pose_aa"]).max()) > 1000 * 4 * ERR["export", "pose_aa"]
        # whole envs, the last env first
        export_against_model(dev, c, rb, dof, [(e, 0, SC.REC_STEPS) for e in reversed(range(SC.REC_ENVS))], upright, "envs in reverse order")
        if upright:                                              # dof_pos absent, out_pose_aa the only optional output: the bits of the full run
            sub = run_export(dev, c, rb, dof, segs, outputs=("out_rot", "out_trans", "out_pose_aa"), use_dof=False)
            for k in sub:
                assert np.array_equal(bits(sub[k]), bits(got[k])), k


# ------------------------------------------------------------------------------------------------------------------ keypoint push
class Stream:
    """The kernel's state and outputs for N envs of J bodies and history H, guarded; a fresh stream unless ``model`` (a StreamModel) gives the state."""
    STATE = ("root_ring", "body_ring", "prev_pos", "count")

    def __init__(self, dev, c, history, envs, model=None):
        self.c, self.h, self.n, self.dev = c, history, envs, dev
        j = c["j"]
        shapes = {"root_ring": (history, 3), "body_ring": (history, j, 3), "prev_pos": (j, 3), "pos": (j, 3), "vel": (j, 3), "raw": (j, 3), "count": ()}
        self.g = Guarded(dev, envs, shapes, {"count": torch.int32})
        v = self.view = self.g.view
        for k in self.STATE:                                      # the outputs stay poison until written
            v[k].zero_()
        if model is not None:
            for k in ("root_ring", "body_ring", "prev_pos"):
                v[k].copy_(torch.from_numpy(getattr(model, k).astype(np.float32)))
        self.taps = torch.from_numpy(kernels.keypoint_taps(history=history)).float().to(dev)

    def push(self, frame, env_mask=None, expand=False):
        j = self.c["j"]
        if expand:                                                # one env's keypoints for every env: env stride 0
            big = torch.full((1, j + 3, 5), float("nan"), device=self.dev)
            big[:, 2:2 + j, 1:4] = torch.from_numpy(frame[:1])
            j3d = big[:, 2:2 + j, 1:4].expand(self.n, j, 3)
            assert j3d.stride(0) == 0
        else:                                                     # a strided view of a NaN-filled buffer
            big = torch.full((self.n + 2, j + 3, 5), float("nan"), device=self.dev)
            j3d = big[1:1 + self.n, 2:2 + j, 1:4]
            j3d.copy_(torch.from_numpy(frame))
        assert j3d.stride(-1) == 1 and not j3d.is_contiguous()
        v = self.view
        kernels.keypoint_push(j3d, taps=self.taps, root_ring=v["root_ring"], body_ring=v["body_ring"], count=v["count"], prev_pos=v["prev_pos"],
                              pos=v["pos"], vel=v["vel"], raw=v["raw"], joint_map=self.c["joint_map"], parents=self.c["parents"],
                              env_mask=None if env_mask is None else torch.as_tensor(env_mask, device=self.dev))
        torch.cuda.synchronize()
        return v["pos"].cpu().numpy(), v["vel"].cpu().numpy()

    def state(self):
        return {k: v.cpu().numpy().copy() for k, v in self.view.items()}


def push_both(s, m, frame, what, envs=None, **kw):
    """One frame through the kernel and the fp64 model; pos, vel at 4 x err on ``envs`` (all), raw bit for bit."""
    pos, vel = s.push(frame, **kw)
    sent = np.broadcast_to(frame[:1], frame.shape) if kw.get("expand") else frame
    want_p, want_v = m.push(sent, env_mask=kw.get("env_mask"))
    sel = slice(None) if envs is None else envs
    hold("keypoint", "pos", pos[sel], want_p[sel], f"{what} pos")
    hold("keypoint", "vel", vel[sel], want_v[sel], f"{what} vel")
    raw = s.view["raw"].cpu().numpy()
    assert np.array_equal(bits(raw[sel]), bits(sent[:, s.c["joint_map"]][sel])), f"{what}: raw is no copy"
    return pos, vel


@pytest.mark.parametrize("kind", SC.TREES)
def test_keypoint_every_tree_body_count_history_and_env_count(dev, kind):
    for c, h, n, pushes in SC.keypoint_streams(kind):
        frames, _ = SC.keypoint_frames(c, n, pushes)
        s, m = Stream(dev, c, h, n), SC.keypoint_model(c, h, n, np.float64)
        what = f"keypoint {kind} J = {c['j']} H = {h} N = {n}"
        for t, f in enumerate(frames):
            push_both(s, m, f, f"{what} push {t}")
        s.g.check(what)
        assert s.view["count"].tolist() == [pushes] * n
        if pushes < h:                                            # the slots no push has reached: still the zeros they were
            assert not s.view["root_ring"][:, pushes:].cpu().view(torch.int32).any() and not s.view["body_ring"][:, pushes:].cpu().view(torch.int32).any()
    assert (c["j"], h, pushes) == (31 if kind != "smpl" else 24, 64, 67)                  # the last stream wrapped the longest ring


@pytest.mark.parametrize("kind,j,history", [("random", 31, 30), ("late_low", 7, 7)])
def test_keypoint_count_near_two_to_the_thirty(dev, kind, j, history):
    """Env 0 of a running stream is at count 2^30 - 2: the kernel rewrites the count it stores to H + count % H, the model counts on without bound.
    2^30 % 30 = 4 and 2^30 % 7 = 1: a rewrite to H alone would move the slot."""
    c, n, big = SC.case("keypoint", kind, j), 3, 2 ** 30 - 2
    assert (2 ** 30) % history != 0
    fill = history + 5
    frames, _ = SC.keypoint_frames(c, n, fill + 4, salt=1)
    m = SC.keypoint_model(c, history, n, np.float64)
    m.count[0] = big - fill
    for f in frames[:fill]:
        m.push(f)
    for k in ("root_ring", "body_ring", "prev_pos"):              # the state both sides start from, as float32 holds it
        setattr(m, k, getattr(m, k).astype(np.float32).astype(np.float64))
    s = Stream(dev, c, history, n, model=m)
    s.view["count"].copy_(torch.tensor([big, fill, fill], dtype=torch.int32))
    assert m.count.tolist() == [big, fill, fill]
    stored = big
    for t, f in enumerate(frames[fill:]):
        push_both(s, m, f, f"keypoint {kind} J = {j} H = {history} count 2^30 - 2 + {t}")
        stored = stored + 1 if stored + 1 < 2 ** 30 else history + (stored + 1) % history
        count = s.view["count"].tolist()
        assert count[0] >= history and count[0] % history == int(m.count[0]) % history, (t, count)
        assert count == [stored, fill + t + 1, fill + t + 1], (t, count)
    assert stored < 2 * history                                  # the rewrite happened
    s.g.check("preset counts")


def test_keypoint_negative_count_is_count_zero(dev):
    c, h, n = SC.case("keypoint", "star", 30), 30, 3
    frames, _ = SC.keypoint_frames(c, n, 3, salt=2)
    s, m = Stream(dev, c, h, n), SC.keypoint_model(c, h, n, np.float64)
    s.view["count"].copy_(torch.tensor([0, -5, 0], dtype=torch.int32))
    for t, f in enumerate(frames):
        push_both(s, m, f, f"keypoint count -5, push {t}")
        assert s.view["count"].tolist() == [t + 1] * n
    s.g.check("negative count")


def test_keypoint_env_stride_zero(dev):
    c, h, n = SC.case("keypoint", "random", 7), 2, 9
    frames, _ = SC.keypoint_frames(c, n, 4, salt=3)
    s, m = Stream(dev, c, h, n), SC.keypoint_model(c, h, n, np.float64)
    for t, f in enumerate(frames):
        push_both(s, m, f, f"keypoint env stride 0, push {t}", expand=True)
        state = s.state()
        for k, v in state.items():                                # equal state in, equal keypoints: equal bits out, env by env
            assert all(np.array_equal(v[e].view(np.int32), v[0].view(np.int32)) for e in range(1, n)), (t, k)
    s.g.check("env stride 0")


def test_keypoint_env_mask_in_the_second_workgroup(dev):
    c, h, n = SC.case("keypoint", "chain", 31), 30, 9
    frames, _ = SC.keypoint_frames(c, n, 6, salt=4)
    s, m = Stream(dev, c, h, n), SC.keypoint_model(c, h, n, np.float64)
    mask = np.ones(n, dtype=bool)
    mask[8] = False                                              # envs 0 .. 7 fill workgroup 0
    for t, f in enumerate(frames):
        masked = t == 0 or 2 <= t < 4                             # at push 0 env 8's outputs are still poison and its state zero: they stay so
        before = s.state()
        push_both(s, m, f, f"keypoint env 8 masked: {masked}, push {t}", envs=np.nonzero(mask)[0] if masked else None, env_mask=mask if masked else None)
        after = s.state()
        if masked:
            for k in before:                                      # all seven buffers of env 8: the bits from before the push; every other env's moved
                assert np.array_equal(before[k][8].view(np.int32), after[k][8].view(np.int32)), (t, k)
                assert all(not np.array_equal(before[k][e].view(np.int32), after[k][e].view(np.int32)) for e in range(8)), (t, k)
    assert s.view["count"].tolist() == [6] * 8 + [3]
    s.g.check("env mask")
