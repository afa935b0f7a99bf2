"""A deterministic family of skeletons other than SMPL's for the three half-wave kernels (pulse_motion_ingest, pulse_motion_export,
pulse_keypoint_push): trees, body counts, joint / mirror maps and inputs, generated from fixed seeds in plain numpy -- no device, nothing stored.
Used by tests/test_half_wave_shapes_cpu.py (the models against an independent statement of the operation, the yardsticks) and
tests/test_half_wave_shapes_gpu.py (the kernels against the models).

  trees        chain [-1, 0, 1, ...]; star (every body on body 0); random (parent[b] drawn from 0 .. b - 1); late_low (a chain whose last two
               bodies hang off body 0 and body 1: the deepest level beside depth-1 and depth-2 bodies with the highest numbers); smpl (SMPL's own
               tree with its own maps: the control)
  body counts  ingest / export J in {1, 2, 6, 23, 25, 31, 32} (no star or random tree at J = 1, late_low from J = 6), keypoint push J in
               {6, 7, 30, 31}; smpl at 24
  maps         ``joint_map`` (export, keypoint push) and ``mirror_map`` (ingest): seeded permutations of 0 .. J - 1 that are NOT their own inverse
               wherever J >= 3 (asserted here, on every case); ``ingest_map`` (ingest): body -> SMPL joint, a seeded subset of the 24 for J < 24,
               all 24 and then repeated joints below the hands for J > 24
  inputs       Gaussian axis-angle poses (sigma 0.8) in float32; recordings of unit rotations (a uniform root, Gaussian axis-angle rotations
               composed down the tree) with Gaussian dof rows; keypoints on a random walk.  Every frame has a seeded stream of its own and is
               redrawn from it while it is not QUIET (below); the redraws are counted by cause and the CPU test bounds them, so that the rule
               cannot turn into a filter.  No frame is left out of a comparison.

A frame is quiet when, with the upright factor on and off,
  * floor: every quaternion whose sign the reference decides has |w| >= 1e-3 (``decided_w`` of the models: the floor the golden fixtures assert);
    for the export also the dump's body_quat (cos(angle / 2): exp_map_to_quat's normalize_angle jumps from pi to -pi where it vanishes) and the
    recorded root's w (quat_to_exp_map's 2 acos w, the same jump), and
  * band: no expected component of a compared field lies in (0, 1e-5): the sibling tests' rule demands that a component within 4 x err of zero be
    an exact zero (a sign the bound cannot keep), and 1e-5 is above 4 x err of every field (asserted by the CPU test).  ``settled``: what the
    fp64 model leaves below 1e-14 where the reference means an exact zero IS that zero.
"""
import os

import numpy as np

import keypoint_stream_model as KM
import motion_export_model as MX
import motion_ingest_model as MI
from pulse_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "half_wave_shapes.txt")

TREES = ("chain", "star", "random", "late_low", "smpl")
KERNELS = ("ingest", "export", "keypoint")
FRAMES = 19                                   # frames per ingest clip, one-frame segments per export case
W_FLOOR = 1e-3
ZERO_BAND = 1e-5
RESIDUE = 1e-14
SIGMA = 0.8
ROOT_OFFSET = np.array([0.1, -0.2, 0.3], dtype=np.float32)
REC_STEPS, REC_ENVS = 4, 5                    # the export recording: 20 (step, env) frames
HISTORIES, ENV_COUNTS = (1, 2, 30, 64), (1, 8, 9)
MIN_LIMB = 0.05                               # metres: the shortest limb a keypoint frame may have
# the fields each kernel is held to (the model's names), and the copies among them (bit for bit)
FIELDS = {"ingest": ("pose_quat_global", "root_trans_offset", "pose_quat", "pose_aa", "trans_orig"),
          "export": ("pose_quat_global", "root_trans_offset", "pose_quat", "pose_aa", "trans_orig", "body_quat", "dof_pos"),
          "keypoint": ("pos", "vel")}
COPIES = {"ingest": ("pose_aa", "trans_orig"), "export": ("pose_quat_global", "root_trans_offset", "dof_pos"), "keypoint": ()}
# where the golden fixture of the kernel stores err of the same field
FIXTURE = {"ingest": "motion_ingest.npz", "export": "motion_export.npz", "keypoint": "keypoint_stream.npz"}
FIXTURE_KEY = {("export", "body_quat"): "err_states_body_quat", ("export", "dof_pos"): "err_states_dof_pos"}


def _rng(*key):
    return np.random.default_rng([KERNELS.index(k) if k in KERNELS else TREES.index(k) if k in TREES else int(k) for k in key])


def body_counts(kernel, kind):
    if kind == "smpl":
        return (24,)
    counts = (6, 7, 30, 31) if kernel == "keypoint" else (1, 2, 6, 23, 25, 31, 32)
    return tuple(j for j in counts if j >= {"chain": 1, "star": 2, "random": 2, "late_low": 6}[kind])


def parents_of(kind, j):
    if kind == "smpl":
        assert j == 24
        return list(syn.SMPL_PARENTS)
    if kind == "chain":
        return list(range(-1, j - 1))
    if kind == "star":
        return [-1] + [0] * (j - 1)
    if kind == "random":
        g = _rng("ingest", kind, j, 1)
        return [-1] + [int(g.integers(0, b)) for b in range(1, j)]
    assert kind == "late_low" and j >= 6
    return list(range(-1, j - 3)) + [0, 1]


def inverse(perm):
    inv = [0] * len(perm)
    for b, s in enumerate(perm):
        inv[s] = b
    return inv


def _permutation(g, j):
    """A permutation of 0 .. j - 1 that is not its own inverse (j >= 3)."""
    while True:
        p = [int(v) for v in g.permutation(j)]
        if j < 3 or p != inverse(p):
            return p


def _ingest_map(g, j):
    order = [int(v) for v in g.permutation(MI.SMPL_JOINTS)]
    return order[:j] + [int(v) for v in g.integers(0, MI.HAND_COL // 3, size=max(0, j - MI.SMPL_JOINTS))]


def case(kernel, kind, j):
    """parents, joint_map (export, keypoint push), ingest_map (ingest's body -> SMPL joint) and mirror_map of one skeleton."""
    c = {"kernel": kernel, "kind": kind, "j": j, "parents": parents_of(kind, j)}
    if kind == "smpl":
        c.update(joint_map=syn.smpl_joint_map(), ingest_map=syn.smpl_joint_map(), mirror_map=syn.mirror_body_map())
        return c
    c.update(joint_map=_permutation(_rng(kernel, kind, j, 2), j), ingest_map=_ingest_map(_rng(kernel, kind, j, 3), j),
             mirror_map=_permutation(_rng(kernel, kind, j, 4), j))
    for name in ("joint_map", "mirror_map"):
        assert sorted(c[name]) == list(range(j))
        assert j < 3 or c[name] != inverse(c[name]), f"{kernel} {kind} J = {j}: {name} is its own inverse: the case has lost its point"
    assert all(0 <= s < MI.SMPL_JOINTS for s in c["ingest_map"]) and len(c["ingest_map"]) == j
    assert len(set(c["ingest_map"])) == min(j, MI.SMPL_JOINTS) and all(s < MI.HAND_COL // 3 for s in c["ingest_map"][MI.SMPL_JOINTS:])
    return c


def cases(kernel, kind):
    return [case(kernel, kind, j) for j in body_counts(kernel, kind)]


def settled(a):
    """An fp64 result with its rounding residue of exact zeros removed: a body whose local rotation is the identity (ingest zeroes the hand joints)
    takes its parent's global rotation, and where normalising that once more moves its last bit, the local rotation recovered from the two
    carries 1e-17 where the reference means 0.  Below RESIDUE (fp64 rounding, a hundred million times under fp32's) a component is that zero."""
    return np.where(np.abs(a) < RESIDUE, 0.0, a)


def _off_zero(*arrays):
    """No component in (0, ZERO_BAND), per frame (the leading axis)."""
    ok = None
    for a in arrays:
        a = np.abs(settled(a).reshape(a.shape[0], -1))
        q = ~((a > 0) & (a < ZERO_BAND)).any(1)
        ok = q if ok is None else ok & q
    return ok


def _floor(w, frames):
    return (w.reshape(frames, -1) >= W_FLOOR).all(1) if w.size else np.ones(frames, dtype=bool)


def _redraw(draw, quiet, frames):
    """``draw(g)`` -> a tuple of arrays of ONE item (frame) from generator g; ``quiet(*stacked)`` -> two (n,) bools (floor met, band met).
    Every item has a generator of its own (``frames``: the list of them) and is redrawn from it while it is not quiet
    -> (stacked arrays, {"floor": redraws, "band": redraws}): a draw that misses the floor counts there, one that only sits in the band, there."""
    data = [np.stack(a) for a in zip(*[draw(g) for g in frames])]
    redraws = {"floor": 0, "band": 0}
    while True:
        floor, band = quiet(*data)
        bad = np.nonzero(~(floor & band))[0]
        if not len(bad):
            return data, redraws
        assert sum(redraws.values()) < 10 * len(frames), "the quiet rule rejects nearly everything"
        for i in bad:
            redraws["band" if floor[i] else "floor"] += 1
            for a, b in zip(data, draw(frames[i])):
                a[i] = b


# ------------------------------------------------------------------------------------------------------------------ ingest
def ingest_model(c, poses, trans, **kw):
    return MI.ingest_clip(poses, trans, 30.0, c["parents"], c["ingest_map"], root_offset=ROOT_OFFSET, mirror_map=c["mirror_map"], **kw)


def ingest_inputs(c):
    """poses (FRAMES, 72) and trans (FRAMES, 3), float32, the hand columns non-zero going in -> (poses, trans, redraws)."""
    def draw(g):
        return (SIGMA * g.standard_normal(72)).astype(np.float32), g.standard_normal(3).astype(np.float32)

    def quiet(poses, trans):
        n = len(poses)
        floor, band = np.ones(n, dtype=bool), np.ones(n, dtype=bool)
        for upright in (True, False):
            res = ingest_model(c, poses, trans, upright_start=upright)
            floor &= _floor(np.abs(res["global_products"][:, 1:, 3]), n) & _floor(np.abs(res["local_products"][:, 1:, 3]), n)     # decided_w, per frame
            band &= _off_zero(res["pose_quat_global"], res["pose_quat"], res["root_trans_offset"])
        return floor, band
    # (stream 15, not 5: at 5 the chain of 31 bodies needed 2 redraws in its 19 frames, one more than the bound the CPU test puts on a case)
    (poses, trans), redraws = _redraw(draw, quiet, [_rng("ingest", c["kind"], c["j"], 15, f) for f in range(FRAMES)])
    return poses, trans, redraws


# ------------------------------------------------------------------------------------------------------------------ export
def export_model(c, rb, dof, **kw):
    return MX.export_frames(rb, dof, c["parents"], c["joint_map"], root_offset=ROOT_OFFSET, **kw)


def export_inputs(c, identity_joints=()):
    """A recording rb (REC_STEPS, REC_ENVS, J, 13) and dof_pos (.., 3 (J - 1)), float32 -> (rb, dof_pos, redraws).  The root's rotation is uniform
    on the sphere; every other body's is its parent's times a Gaussian axis-angle rotation (sigma 0.8), composed in fp64 and rounded to float32
    as a recording holds it; positions, velocities and dof rows Gaussian.  ``identity_joints``: the bodies whose joint_map entry is among them
    take their parent's rotation (an identity local rotation)."""
    j = c["j"]

    def draw(g):
        rb = g.standard_normal((j, 13))
        rb[0, 3:7] /= np.linalg.norm(rb[0, 3:7])
        local = MI.from_rotvec(SIGMA * g.standard_normal((j, 3)))
        for b in range(1, j):
            rb[b, 3:7] = rb[c["parents"][b], 3:7] if c["joint_map"][b] in identity_joints else MI.quat_mul(rb[c["parents"][b], 3:7], local[b])
        return rb.astype(np.float32), (SIGMA * g.standard_normal(3 * (j - 1))).astype(np.float32)

    def quiet(rb, dof):
        n = len(rb)
        floor, band = _floor(np.abs(rb[:, 0, 6]), n), np.ones(n, dtype=bool)
        for upright in (True, False):
            res = export_model(c, rb, dof, upright_start=upright)
            if upright:
                floor &= _floor(np.abs(res["local_products"][:, 1:, 3]), n)
            floor &= _floor(np.abs(res["pose_quat"][..., 3]), n) & _floor(np.abs(res["body_quat"][..., 3]), n)
            band &= _off_zero(res["pose_quat"], res["pose_aa"], res["trans_orig"], res["body_quat"])
        return floor, band
    gens = [_rng("export", c["kind"], c["j"], 7 if identity_joints else 6, f) for f in range(REC_STEPS * REC_ENVS)]
    (rb, dof), redraws = _redraw(draw, quiet, gens)
    return rb.reshape(REC_STEPS, REC_ENVS, j, 13), dof.reshape(REC_STEPS, REC_ENVS, 3 * (j - 1)), redraws


def one_frame_segments(c):
    """FRAMES one-frame segments (env, t0, 1) of the recording in a seeded order: every output frame is a segment of its own, and a wrong
    segment looked up for it reads another (step, env)."""
    g = _rng("export", c["kind"], c["j"], 8)
    return [(int(i) % REC_ENVS, int(i) // REC_ENVS, 1) for i in g.permutation(REC_STEPS * REC_ENVS)[:FRAMES]]


# ------------------------------------------------------------------------------------------------------------------ keypoint push
def keypoint_frames(c, envs, pushes, salt=0):
    """(pushes, envs, J, 3) float32 keypoints: a random pose per env around a root up to a few metres out, on a random walk; every limb
    (body 1 .. 5 to its parent, after the reordering) at least MIN_LIMB long in every frame -> (frames, redraws); an env is drawn and redrawn whole."""
    j = c["j"]

    def draw(g):
        base = 0.5 * g.standard_normal((1, j, 3)) + 2.0 * g.standard_normal((1, 1, 3))
        return ((base + np.cumsum(0.02 * g.standard_normal((pushes, j, 3)), axis=0)).astype(np.float32),)

    def quiet(f):
        p = f.astype(np.float64)[:, :, c["joint_map"]]
        limb = np.stack([np.linalg.norm(p[:, :, c["parents"][i]] - p[:, :, i], axis=-1) for i in range(1, KM.LIMBS + 1)], axis=-1)
        return (limb >= MIN_LIMB).all((1, 2)), np.ones(len(f), dtype=bool)
    (f,), redraws = _redraw(draw, quiet, [_rng("keypoint", c["kind"], j, 9, envs, pushes, salt, e) for e in range(envs)])
    return np.ascontiguousarray(f.transpose(1, 0, 2, 3)), redraws


def keypoint_streams(kind):
    """(case, history, envs, pushes) of every stream the GPU test runs on this tree: H + 3 pushes capped at 12, one H = 64 stream run to 67 so
    that the ring wraps."""
    out = []
    for c in cases("keypoint", kind):
        for h in HISTORIES:
            for n in ENV_COUNTS:
                out.append((c, h, n, min(h + 3, 12)))
    out.append((cases("keypoint", kind)[-1], 64, 2, 67))
    return out


def keypoint_model(c, history, envs, dtype):
    return KM.StreamModel(envs, history=history, joint_map=c["joint_map"], parents=c["parents"], dtype=dtype)


# ------------------------------------------------------------------------------------------------------------------ the yardsticks
def _gap(a32, a64):
    return float(np.abs(a32.astype(np.float64) - a64).max()) if a64.size else 0.0


def family_err():
    """{(kernel, field): max |model(float32) - model(float64)| over the whole family}: the error of an fp32 evaluation of the reference's own
    statements on these skeletons.  Upright factor on and off, the mirrored copy, every stream of ``keypoint_streams``."""
    err = {(k, f): 0.0 for k in KERNELS for f in FIELDS[k]}

    def take(kernel, r32, r64):
        for f in FIELDS[kernel]:
            err[kernel, f] = max(err[kernel, f], _gap(r32[f], r64[f]))
    for kind in TREES:
        for c in cases("ingest", kind):
            poses, trans, _ = ingest_inputs(c)
            for kw in ({"upright_start": True}, {"upright_start": False}, {"upright_start": True, "mirror": True}):
                take("ingest", ingest_model(c, poses, trans, dtype=np.float32, **kw), ingest_model(c, poses, trans, **kw))
        for c in cases("export", kind):
            rb, dof, _ = export_inputs(c)
            rb, dof = rb.reshape(-1, c["j"], 13), dof.reshape(REC_STEPS * REC_ENVS, 3 * (c["j"] - 1))
            for upright in (True, False):
                take("export", export_model(c, rb, dof, upright_start=upright, dtype=np.float32), export_model(c, rb, dof, upright_start=upright))
        for c, h, n, pushes in keypoint_streams(kind):
            frames, _ = keypoint_frames(c, n, pushes)
            m32, m64 = keypoint_model(c, h, n, np.float32), keypoint_model(c, h, n, np.float64)
            for f in frames:
                m32.push(f)
                m64.push(f)
                take("keypoint", m32.state(), m64.state())
    return err


def fixture_err():
    """{(kernel, field): err of the same field as the kernel's golden fixture stores it}."""
    out = {}
    for k in KERNELS:
        z = np.load(os.path.join(ROOT, "tests", "golden", FIXTURE[k]))
        for f in FIELDS[k]:
            out[k, f] = float(z[FIXTURE_KEY.get((k, f), "err_" + f)])
    return out


def yardsticks():
    """{(kernel, field): (err_field, source)}: the family maximum floored at the fixture's figure."""
    fam, fix = family_err(), fixture_err()
    return {k: (max(fam[k], fix[k]), "family" if fam[k] > fix[k] else "fixture") for k in fam}


def stored_yardsticks(path=PROFILE):
    """The ``err`` lines of profiles/half_wave_shapes.txt -> {(kernel, field): (err_field, source, worst measured ratio or None)}."""
    out = {}
    with open(path) as fh:
        for line in fh:
            w = line.split()
            if len(w) >= 8 and w[0] == "err" and w[1] in KERNELS:
                out[w[1], w[2]] = (float(w[3]), w[5], None if w[7] == "-" else float(w[7]))
    return out


def format_yardsticks(ys, ratios=None):
    """The lines ``stored_yardsticks`` reads: err <kernel> <field> <err_field> source <family|fixture> worst <ratio|->."""
    ratios = ratios or {}
    return "".join(f"err {k:<8} {f:<17} {e!r:<23} source {s:<7} worst {ratios.get((k, f), '-')}\n" for (k, f), (e, s) in ys.items())
