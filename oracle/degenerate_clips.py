"""Degenerate motion clips for the motion-query kernels (ORACLE / TEST INFRASTRUCTURE -- never imported by pulse_amd).

Real clips hold what the synthetic libraries never do: joints that do not move at all (identical bits on every frame), joints whose
local rotation is exactly the identity (the SMPL hands), joints that creep by less than a milliradian per frame, quaternions that
change hemisphere between frames, clips of 2 or 3 frames.  ``build`` makes a small library of such clips in the table layout of
``pulse_amd.synthetic.synthetic_motion_library``; ``queries`` the (motion id, time) pairs that hit every frame, blend and clip edge.

Why a predicate.  The reference's slerp (phc/utils/torch_utils.py:175-197) picks among three results -- q0, 0.5 q0 + 0.5 q1, the
general form -- by thresholds on the fp32 dot product of the pair.  For a slow joint the choice turns on the last bits of that dot
product, hence on the ORDER in which its four products are added: torch's CPU sum is one order, a left-to-right device sum another, and
the two legitimately disagree by up to 0.5 |q1 - q0| per component (profiles/motion_degenerate_branches.txt).  ``classify`` evaluates
the dot product in every order a sane implementation may use, moves each value by up to 2 ulp, and calls a pair STABLE only when every
evaluation takes the same branch.  ``build`` keeps only stable pairs (slow pairs are redrawn until they are) and asserts it of every
consecutive pair of ``lrs`` and ``grs``; ``query_conditions`` does the same for the two cliffs of quat_to_angle_axis.  These are
conditions on the INPUTS; no comparison of a kernel with the reference is skipped or loosened because of them.
"""
import numpy as np
import torch

from pulse_amd import synthetic as syn
from . import rotations as R
from .motion_oracle import OracleMotionLib

# branch of slerp a pair takes; + FLIP when the dot product is negative (q1 is negated first)
Q0, MID, GEN, IDENT = 0, 1, 2, 3
FLIP = 4
BRANCH_NAMES = ("q0", "midpoint", "general", "identity-masked")

# joint kinds
MOVING, FROZEN, IDENTITY, SLOW, FLIPPED, FLIPPED_ALT = 0, 1, 2, 3, 4, 5
KIND_NAMES = ("moving", "frozen", "identity", "slow", "flipped", "flipped-alternate")

MIN_ABS_DOT = 1e-3               # |c| floor of a stable pair: the flip decision is not left to round-off
MOVING_MIN_HALF_ANGLE = 4e-3     # a moving pair is at least this far apart: sqrt(1 - c c) >= 4e-3, four times the midpoint threshold
SLOW_HALF_ANGLE = (6.5e-4, 8.5e-4)
ULP_SHIFTS = (-2, -1, 0, 1, 2)
MIN_SIN2 = 1e-6                  # query_conditions: 1 - w w of an interpolated dof joint is exactly 0 or at least this (mask at 1e-5 ** 2 = 1e-10)
MIN_ABS_W = 1e-2                 # ... and |w| stays clear of the wrap of 2 acos w at pi

# (frames, fps, what): eight clips, frame counts {2, 3, 9, 17} at both rates
CLIPS = ((2, 30.0, "mixed"), (3, 60.0, "mixed"), (9, 30.0, "still"), (17, 60.0, "stretch"), (9, 60.0, "root-flipped"), (17, 30.0, "alternate"),
         (2, 60.0, "mixed"), (3, 30.0, "root-slow"))
STRETCH = (5, 9)                 # the "stretch" clip holds the bits of frame 5 on frames 5 .. 9

_F32 = np.float32


def tree(humanoid):
    """The description ``syn.skeleton`` returns; an integer J stands for a binary tree of J bodies (parent of b: (b - 1) // 2)."""
    if isinstance(humanoid, int):
        return {"parents": [-1] + [(b - 1) // 2 for b in range(1, humanoid)], "body_names": [f"b{b}" for b in range(humanoid)]}
    return syn.skeleton(humanoid)


# ------------------------------------------------------------------------------------------------------------------------------
# the stability predicate
# ------------------------------------------------------------------------------------------------------------------------------
def dot_forms(q0, q1):
    """The fp32 dot product of (..., 4) float32 arrays in five forms: three association orders, torch.sum, fp64 rounded to fp32."""
    q0, q1 = np.ascontiguousarray(q0, dtype=_F32), np.ascontiguousarray(q1, dtype=_F32)
    p = q0 * q1
    x, y, z, w = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    return [((x + y) + z) + w, (x + y) + (z + w), (x + z) + (y + w), torch.sum(torch.from_numpy(p), dim=-1).numpy(),
            (q0.astype(np.float64) * q1.astype(np.float64)).sum(-1).astype(_F32)]


def branch_of(c):
    """Branch of slerp for the fp32 dot product ``c``, in fp32 like the reference: Q0 | MID | GEN, + FLIP when c < 0."""
    c = np.asarray(c, dtype=_F32)
    a = np.abs(c)
    with np.errstate(invalid="ignore"):
        sh = np.sqrt(_F32(1.0) - a * a)
    b = np.where(a >= _F32(1.0), Q0, np.where(np.abs(sh) < _F32(0.001), MID, GEN))
    return (b + FLIP * (c < 0)).astype(np.int64)


def _shift(c, k):
    for _ in range(abs(k)):
        c = np.nextafter(c, _F32(np.inf if k > 0 else -np.inf))
    return c


def classify(q0, q1):
    """(stable, label) of every pair of the (..., 4) float32 arrays.  ``label``: the branch of the left-to-right dot product (+ FLIP); a pair
    of identical bits is Q0 whatever its dot product rounds to (all three branches return q0 exactly), IDENT when it is (0, 0, 0, +-1)."""
    q0, q1 = np.ascontiguousarray(q0, dtype=_F32), np.ascontiguousarray(q1, dtype=_F32)
    forms = dot_forms(q0, q1)
    label = branch_of(forms[0])
    same = np.ones(label.shape, dtype=bool)
    min_abs = np.full(label.shape, np.inf)
    for c in forms:
        min_abs = np.minimum(min_abs, np.abs(c))
        for k in ULP_SHIFTS:
            same &= branch_of(_shift(c, k)) == label
    identical = (q0.view(np.uint32) == q1.view(np.uint32)).all(-1)
    stable = identical | (same & (min_abs > MIN_ABS_DOT))
    ident = identical & (q0[..., :3] == 0).all(-1)
    label = np.where(identical, np.where(ident, IDENT, Q0), label)
    return stable, label


def draw_pairs(rng, n, h):
    """n pairs WITHOUT the predicate: q0 uniform on the sphere, q1 = dq q0 with dq a rotation of half-angle h about a uniform axis (fp64,
    rounded to fp32; h = 0: the same bits).  What tools/motion_degenerate_branches.py tabulates."""
    q0 = rng.standard_normal((n, 4))
    q0 /= np.linalg.norm(q0, axis=-1, keepdims=True)
    axis = rng.standard_normal((n, 3))
    ax, ay, az = (axis / np.linalg.norm(axis, axis=-1, keepdims=True) * np.sin(h)).T
    aw = np.full(n, np.cos(h))
    bx, by, bz, bw = q0.T
    q1 = np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                   aw * bw - ax * bx - ay * by - az * bz], axis=-1)
    q1 /= np.linalg.norm(q1, axis=-1, keepdims=True)
    q0 = q0.astype(_F32)
    return q0, (q0 if h == 0.0 else q1.astype(_F32))


def pair_labels(tables):
    """For the flat frame index f: (stable, label) of the pair (f, next frame of the same clip, the last frame paired with itself) of
    ``lrs`` and ``grs``, each (F, J), and ``pair_rows`` (F,): False on the last frame of every clip.  A query whose first frame is f
    interpolates exactly this pair."""
    nf, starts = tables["motion_num_frames"], tables["length_starts"]
    total = tables["lrs"].shape[0]
    mid = torch.repeat_interleave(torch.arange(nf.shape[0]), nf)
    last = starts[mid] + nf[mid] - 1
    nxt = torch.minimum(torch.arange(total) + 1, last).numpy()
    out = {"pair_rows": (torch.arange(total) < last).numpy()}
    for k in ("lrs", "grs"):
        q = tables[k].numpy()
        out[k + "_stable"], out[k + "_labels"] = classify(q, q[nxt])
    return out


def unstable_pairs(tables):
    """[(table, flat frame, body)] of the consecutive pairs that fail ``classify``."""
    lab = pair_labels(tables)
    return [(k, int(f), int(b)) for k in ("lrs", "grs") for f, b in zip(*np.nonzero(~lab[k + "_stable"]))]


def query_conditions(tables, ids, times):
    """Violations [(query, dof joint, w)] of the two conditions under which quat_to_angle_axis has no cliff near the interpolated local
    rotation (evaluated in fp64): 1 - w w is exactly 0 (an identity joint: masked whatever the rounding) or >= MIN_SIN2 (the mask
    |sin| > 1e-5 holds whatever the rounding), and |w| >= MIN_ABS_W.  Callers assert the list empty."""
    lib = OracleMotionLib({k: v for k, v in tables.items() if isinstance(v, torch.Tensor)})
    f0, f1, blend = lib._frames(ids, times)
    q = R.slerp(lib.lrs[f0].double(), lib.lrs[f1].double(), blend.double()[:, None, None])[:, 1:]
    w = q[..., 3]
    s2 = 1.0 - w * w
    bad = ~((s2 == 0) | (s2 >= MIN_SIN2)) | (w.abs() < MIN_ABS_W)
    return [(int(i), int(d), float(w[i, d])) for i, d in torch.nonzero(bad).tolist()]


# ------------------------------------------------------------------------------------------------------------------------------
# the clips
# ------------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _quat(e):
    """xyzw of the exp map e, fp64."""
    ang = np.linalg.norm(e, axis=-1, keepdims=True)
    return _unit(np.concatenate([e / ang * np.sin(0.5 * ang), np.cos(0.5 * ang)], axis=-1))


def _qmul64(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def _frozen(rng):
    """One rotation by 0.4 .. 2.5 rad: not the identity, |w| <= 0.99, clear of the wrap at pi."""
    return _quat(_unit(rng.standard_normal(3)) * rng.uniform(0.4, 2.5)).astype(_F32)


def _root_e0(rng):
    """Exp map of a root that stands roughly upright: a yaw of 0.9 .. 1.3 rad either way under a tilt of a few tenths, so that the heading
    (atan2 of the horizontal projection of its x axis, which the AMP frame and the task resets take) stays well defined."""
    return np.array([0.15 * rng.standard_normal(), 0.15 * rng.standard_normal(), rng.choice([-1.0, 1.0]) * rng.uniform(0.9, 1.3)])


def _moving(rng, n, root=False):
    """n rotations, consecutive ones 0.04 .. 0.1 rad apart; the exp map keeps 0.9 .. 2.1 rad from the identity (the root: yaws on)."""
    if root:
        e0 = _root_e0(rng)
        d = np.array([0.01 * rng.standard_normal(), 0.01 * rng.standard_normal(), np.sign(e0[2]) * rng.uniform(0.04, 0.10)])
    else:
        e0 = _unit(rng.standard_normal(3)) * rng.uniform(0.9, 1.3)
        d = rng.standard_normal(3)
        d = _unit(d - e0 * (d @ e0) / (e0 @ e0)) * rng.uniform(0.04, 0.10)
    e = e0 + d * np.arange(n)[:, None] + 0.005 * rng.standard_normal((n, 3))
    return _quat(e).astype(_F32)


def _slow(rng, n, root=False):
    """n rotations, consecutive ones a half-angle in SLOW_HALF_ANGLE apart; every pair is redrawn until it is stable on the midpoint branch."""
    q = [_quat(_root_e0(rng)).astype(_F32) if root else _frozen(rng)]
    for _ in range(n - 1):
        for _try in range(10000):
            h = rng.uniform(*SLOW_HALF_ANGLE)
            dq = np.concatenate([_unit(rng.standard_normal(3)) * np.sin(h), [np.cos(h)]])
            cand = _unit(_qmul64(dq, q[-1].astype(np.float64))).astype(_F32)
            stable, label = classify(q[-1], cand)
            if stable and label == MID:
                break
        else:
            raise AssertionError("no stable slow pair in 10000 draws")
        q.append(cand)
    return np.stack(q)


def clip_kinds(what, clip, sk):
    """Joint kind of every body of one clip."""
    parents, names = sk["parents"], sk.get("body_names") or []
    j = len(parents)
    hands = [names.index(n) for n in ("L_Hand", "R_Hand") if n in names] or [j - 2, j - 1]
    if what == "still":
        # the root and its first chain hold the exact identity, so that some GLOBAL rotations are the identity too
        chain = {0}
        for b in range(1, j):
            if parents[b] in chain and len(chain) < 3:
                chain.add(b)
        return [IDENTITY if b in chain or b in hands else FROZEN for b in range(j)]
    cycle = (MOVING, FROZEN, SLOW, FLIPPED, IDENTITY, MOVING, SLOW, FROZEN)
    kinds = [MOVING] + [cycle[(b + 3 * clip) % len(cycle)] for b in range(1, j)]
    for b in hands:
        kinds[b] = IDENTITY
    if what == "root-flipped":
        kinds[0] = FLIPPED
    if what == "alternate":
        kinds[kinds.index(FLIPPED)] = FLIPPED_ALT
    if what == "root-slow":
        # a slow root under a slow / frozen child would put the child's GLOBAL pair anywhere below 1.7e-3: the root's children move
        kinds = [SLOW] + [MOVING if parents[b] == 0 else kinds[b] for b in range(1, j)]
    return kinds


def _clip(rng, frames, fps, what, kinds, parents, offsets):
    j = len(parents)
    pose = list(range(frames))
    if what == "stretch":
        a, b = STRETCH
        pose = [p if p <= a else (a if p <= b else p - (b - a)) for p in pose]
    if what == "still":
        pose = [0] * frames
    n = max(pose) + 1
    lrs = np.empty((n, j, 4), dtype=_F32)
    for b, kind in enumerate(kinds):
        if kind == IDENTITY:
            lrs[:, b] = (0.0, 0.0, 0.0, 1.0)
        elif kind == FROZEN:
            lrs[:, b] = _frozen(rng)
        elif kind == SLOW:
            lrs[:, b] = _slow(rng, n, root=b == 0)
        else:
            lrs[:, b] = _moving(rng, n, root=b == 0)
            if kind == FLIPPED:
                lrs[max(1, n // 2):, b] *= -1
            elif kind == FLIPPED_ALT:
                lrs[1::2, b] *= -1
    t = np.arange(n) / fps
    root = (rng.standard_normal(3) * [0.6, 0.6, 0.0]) * t[:, None] + 0.05 * rng.standard_normal(3) * np.sin(3.0 * t)[:, None] + [0.0, 0.0, 0.9]
    zero = what == "still"
    vel = [np.zeros((n, w, 3), dtype=_F32) if zero else rng.standard_normal((n, w, 3)).astype(_F32) for w in (j, j, j - 1)]
    lrs, root = torch.from_numpy(lrs[pose]), torch.from_numpy(root.astype(_F32)[pose])
    grs, gts = torch.empty(frames, j, 4), torch.empty(frames, j, 3)
    for b in range(j):                                                             # the fp32 forward kinematics of synthetic_motion_library
        p = parents[b]
        if p < 0:
            grs[:, b], gts[:, b] = lrs[:, b], root
        else:
            grs[:, b] = syn._quat_mul_xyzw(grs[:, p], lrs[:, b])
            gts[:, b] = gts[:, p] + syn._quat_rotate_xyzw(grs[:, p], offsets[b].expand(frames, 3))
    grs = grs / grs.norm(dim=-1, keepdim=True)
    gvs, gavs, dvs = (torch.from_numpy(v[pose]) for v in vel)
    return {"gts": gts, "grs": grs, "lrs": lrs, "gvs": gvs, "gavs": gavs, "dvs": dvs}


def _tables(clips, fields):
    nf = torch.tensor([c[0] for c in clips], dtype=torch.int64)
    fps = torch.tensor([c[1] for c in clips], dtype=torch.float32)
    tabs = {k: torch.cat([f[k] for f in fields]).contiguous() for k in ("gts", "grs", "lrs", "gvs", "gavs", "dvs")}
    tabs.update({"motion_num_frames": nf, "motion_fps": fps, "motion_dt": (1.0 / fps.double()).float(),
                 "motion_lengths": ((1.0 / fps.double()) * (nf - 1).double()).float(), "length_starts": torch.cumsum(nf, 0) - nf})
    return tabs


def build(seed, humanoid="smpl", clips=CLIPS):
    """(tables, info): the library, and ``info`` = pair_labels(tables) + ``kinds`` (M, J) + ``clips``.  Every consecutive pair of lrs and of grs
    of every body is asserted stable: slow local pairs are redrawn one by one, a clip whose GLOBAL pairs fail (a slow root under the fp32
    forward kinematics, a chance cancellation) is redrawn whole."""
    sk = tree(humanoid)
    parents = sk["parents"]
    j = len(parents)
    rng0 = np.random.default_rng([seed, j])
    offsets = torch.from_numpy((0.08 + 0.3 * rng0.random((j, 3)) * [0.4, 0.4, 1.0]).astype(_F32))
    offsets[0] = 0.0
    fields, kinds = [], []
    for c, (frames, fps, what) in enumerate(clips):
        kinds.append(clip_kinds(what, c, sk))
        for attempt in range(200):
            cand = _clip(np.random.default_rng([seed, j, c, attempt]), frames, fps, what, kinds[-1], parents, offsets)
            if not unstable_pairs(_tables([clips[c]], [cand])):
                break
        else:
            raise AssertionError(f"clip {c} ({what}): no stable draw in 200")
        fields.append(cand)
    tables = _tables(clips, fields)
    bad = unstable_pairs(tables)
    assert not bad, f"unstable consecutive pairs (table, frame, body): {bad[:8]}"
    info = pair_labels(tables)
    info["kinds"] = np.asarray(kinds, dtype=np.int64)
    info["clips"] = tuple(clips)
    _check_kinds(tables, info)
    return tables, info


def _check_kinds(tables, info):
    """What the joint kinds promise, asserted on the finished tables."""
    lrs, nf, starts = tables["lrs"].numpy(), tables["motion_num_frames"].tolist(), tables["length_starts"].tolist()
    for m, (n, s) in enumerate(zip(nf, starts)):
        q, lab = lrs[s:s + n], info["lrs_labels"][s:s + n - 1]
        what = info["clips"][m][2]
        for b, kind in enumerate(info["kinds"][m]):
            still = np.ones(n - 1, dtype=bool) if what == "still" else np.array([what == "stretch" and STRETCH[0] <= f < STRETCH[1] for f in range(n - 1)])
            if kind == IDENTITY:
                assert (q[:, b] == np.array([0, 0, 0, 1], dtype=_F32)).all() and (lab[:, b] == IDENT).all()
            elif kind == FROZEN:
                assert (q[:, b].view(np.uint32) == q[0, b].view(np.uint32)).all() and abs(q[0, b, 3]) <= 0.99 and (lab[:, b] == Q0).all()
            elif kind == SLOW:
                assert (lab[~still, b] == MID).all() and (lab[still, b] == Q0).all()
            else:
                c = np.abs((q[:-1, b].astype(np.float64) * q[1:, b]).sum(-1))[~still]
                assert (np.sqrt(1.0 - np.minimum(c, 1.0) ** 2) >= MOVING_MIN_HALF_ANGLE).all(), (m, b)
                assert (lab[~still, b] % FLIP == GEN).all()
                if kind != MOVING:
                    assert (lab[:, b] >= FLIP).any(), (m, b)
    if any(c[2] == "still" for c in info["clips"]):
        m = [c[2] for c in info["clips"]].index("still")
        for k in ("gts", "grs", "lrs", "gvs", "gavs", "dvs"):
            t = tables[k][starts[m]:starts[m] + nf[m]]
            assert torch.equal(t, t[:1].expand_as(t)), k
        assert not tables["gvs"][starts[m]].any()


def queries(tables, seed):
    """(motion_ids, motion_times, offset): for every clip every exact frame time k dt (the last frame included), five times inside every
    blend (the middle among them), t < 0 (twice), t = length, one fp32 step below and above it, and t > length."""
    rng = np.random.default_rng([seed, 77])
    ids, times = [], []
    f32 = torch.float32
    for m, (n, dt, length) in enumerate(zip(tables["motion_num_frames"].tolist(), tables["motion_dt"], tables["motion_lengths"])):
        k = torch.arange(n, dtype=f32)
        t = [k * dt]
        for u in (0.5, *rng.uniform(0.05, 0.95, 4)):
            t.append((k[:-1] + float(u)) * dt)
        up, down = torch.nextafter(length, torch.tensor(float("inf"))), torch.nextafter(length, torch.tensor(0.0))
        t.append(torch.stack([torch.tensor(-0.3), -dt * 1e-3, length, down, up, length * 1.2 + 0.1]).to(f32))
        t = torch.cat(t)
        times.append(t)
        ids.append(torch.full((t.numel(),), m, dtype=torch.int64))
    ids, times = torch.cat(ids), torch.cat(times)
    offset = torch.from_numpy((rng.standard_normal((ids.numel(), 3)) * [2.0, 2.0, 0.5]).astype(_F32))
    return ids, times.contiguous(), offset


def cell_labels(tables, info, ids, times):
    """(lrs labels, grs labels), each (n, J): the branch label of the pair every (query, body) cell interpolates."""
    lib = OracleMotionLib(tables)
    f0, f1, _ = lib._frames(ids, times)
    assert torch.equal(f1, torch.minimum(f0 + 1, (tables["length_starts"] + tables["motion_num_frames"] - 1)[ids]))
    return info["lrs_labels"][f0.numpy()], info["grs_labels"][f0.numpy()]


def load_fixture(path):
    """(npz, tables, info) of tests/golden/motion_degenerate.npz (oracle/gen_golden.py: gen_motion_degenerate)."""
    z = np.load(path)
    tabs = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("tab_")}
    info = {k: z[k] for k in ("kinds", "pair_rows", "lrs_labels", "grs_labels")}
    info["clips"] = CLIPS
    return z, tabs, info


def label_counts(labels):
    """{name: count} over a label array: the four branches and 'flip'."""
    labels = np.asarray(labels)
    out = {name: int((labels % FLIP == b).sum()) for b, name in enumerate(BRANCH_NAMES)}
    out["flip"] = int((labels >= FLIP).sum())
    return out
