"""Deterministic (pred, gt) cases for pulse_im_eval_accum (include/pulse_hip.h section 2b''), sorted by what the 3 x 3 matrix H of the Procrustes
fit looks like: its rank, its conditioning, and how many lanes of a group hold a body.  Every case declares its class, and ``conditions``
checks the class on the arrays themselves, on the singular values of every env's and step's H in fp64 numpy.  Not a test module.

Classes with a reference (compared with eval_metrics_ref.accumulator_row):
    generic       sigma3 >= 1e-3 sigma1
    slab          sigma3 / sigma1 in [1e-9, 1e-3): a thin slab, or an exactly planar cloud turned by a generic rotation and rounded to fp32
    gt_planar     one coordinate of the reference bit-identical over all bodies: a zero row of H, sigma3 <= 1e-15 sigma1
    pred_planar   the same for the prediction: a zero column of H
    both_planar   both, on the same axis or on different ones
    three_bodies  J = 3: both centred clouds have rank <= 2
    exact         pred bit-equal to gt, or a similarity transform of it (rotation, scale 1.7, shift) computed in fp64 and rounded to fp32
all of them with sigma2 >= 0.05 sigma1 in every env and step: below that the rotation itself is not determined by the data.

Classes without one (the restatement divides 0 / 0, or its rotation is arbitrary): one_body, two_bodies, gt_collinear, pred_point, gt_point."""
from dataclasses import dataclass

import numpy as np

from tests.eval_metrics_ref import procrustes_fit

REFERENCED = ("generic", "slab", "gt_planar", "pred_planar", "both_planar", "three_bodies", "exact")
UNREFERENCED = ("one_body", "two_bodies", "gt_collinear", "pred_point", "gt_point")
SIGMA2_MIN = 0.05                                 # of sigma1, every referenced class
PLANAR_SIGMA3_MAX = 1e-15                         # of sigma1, the planar classes
SCALE = 1.7                                       # of the similarity transform in "exact"


@dataclass(frozen=True)
class Case:
    name: str
    cls: str
    pred: np.ndarray                              # (T, N, J, 3) float32
    gt: np.ndarray
    mirrored: tuple = ()                          # envs whose prediction is a mirror image of the reference
    gt_axis: tuple = ()                           # per env: the constant coordinate of the reference (None: not planar)
    pred_axis: tuple = ()
    identical: tuple = ()                         # "exact": envs whose prediction is bit-equal to the reference

    def conditions(self):
        return conditions(self)


def singular_values(pred, gt):
    """(T, N, 3) singular values of H, descending, and (T, N) det H, from the root-relative clouds in fp64 as the restatement forms them."""
    p, g = pred.astype(np.float64), gt.astype(np.float64)
    t, n = p.shape[:2]
    sv, det = np.zeros((t, n, 3)), np.zeros((t, n))
    for s in range(t):
        for e in range(n):
            h = procrustes_fit(p[s, e] - p[s, e, :1], g[s, e] - g[s, e, :1])[3]
            sv[s, e], det[s, e] = np.linalg.svd(h, compute_uv=False), np.linalg.det(h)
    return sv, det


def _constant_column(x, axis):
    """The coordinate is bit-identical over the bodies, so the centred fp64 column is exactly zero."""
    col = x[..., axis]
    assert (col.view(np.uint32) == col[..., :1].view(np.uint32)).all()
    c64 = col.astype(np.float64) - col[..., :1].astype(np.float64)          # root-relative, as the kernel and the restatement go on
    assert (c64 - c64.mean(-1, keepdims=True) == 0.0).all()


def conditions(case):
    """Assert what the case's class promises, on the arrays themselves.  Returns the (T, N, 3) singular values (None without a reference)."""
    pred, gt = case.pred, case.gt
    assert pred.dtype == np.float32 and gt.dtype == np.float32 and pred.shape == gt.shape and pred.ndim == 4 and pred.shape[-1] == 3
    assert np.isfinite(pred).all() and np.isfinite(gt).all()
    t, n, j = pred.shape[:3]
    if case.cls in UNREFERENCED:
        pl, gl = pred.astype(np.float64) - pred[:, :, :1], gt.astype(np.float64) - gt[:, :, :1]
        rank_gt = np.linalg.matrix_rank(gl - gl.mean(2, keepdims=True), tol=1e-6)
        rank_pred = np.linalg.matrix_rank(pl - pl.mean(2, keepdims=True), tol=1e-6)
        if case.cls == "one_body":
            assert j == 1
        elif case.cls == "two_bodies":
            assert j == 2
        elif case.cls == "gt_collinear":
            assert j >= 3 and (rank_gt == 1).all()
        elif case.cls == "pred_point":
            assert j >= 3 and (pred == pred[:, :, :1]).all() and (rank_gt >= 2).all()
        elif case.cls == "gt_point":
            assert j >= 3 and (gt == gt[:, :, :1]).all() and (rank_pred >= 2).all()
        return None
    assert case.cls in REFERENCED, case.cls
    sv, det = singular_values(pred, gt)
    ratio3, ratio2 = sv[..., 2] / sv[..., 0], sv[..., 1] / sv[..., 0]
    assert (ratio2 >= SIGMA2_MIN).all(), (case.name, ratio2.min())
    if case.cls == "generic":
        assert (ratio3 >= 1e-3).all(), (case.name, ratio3.min())
    elif case.cls == "slab":
        assert ((ratio3 >= 1e-9) & (ratio3 < 1e-3)).all(), (case.name, ratio3.min(), ratio3.max())
    elif case.cls in ("gt_planar", "pred_planar", "both_planar"):
        assert (ratio3 <= PLANAR_SIGMA3_MAX).all(), (case.name, ratio3.max())
        for e in range(n):
            if case.cls != "pred_planar":
                _constant_column(gt[:, e], case.gt_axis[e])
            if case.cls != "gt_planar":
                _constant_column(pred[:, e], case.pred_axis[e])
        if case.cls == "gt_planar":                                          # the OTHER cloud is not planar: its out-of-plane part is what a rank-2 R drops
            spread = np.stack([pred[:, e, :, case.gt_axis[e]].astype(np.float64).std(-1) for e in range(n)])
            assert (spread > 5e-3).all(), (case.name, spread.min())
            assert len(case.mirrored) >= 1
        if case.cls == "pred_planar":
            spread = np.stack([gt[:, e, :, case.pred_axis[e]].astype(np.float64).std(-1) for e in range(n)])
            assert (spread > 5e-3).all(), (case.name, spread.min())
    elif case.cls == "three_bodies":
        assert j == 3 and (ratio3 <= 1e-12).all(), (case.name, ratio3.max())
    elif case.cls == "exact":
        assert len(case.identical) >= 1 and len(case.identical) < n
        for e in range(n):
            if e in case.identical:
                assert (pred[:, e].view(np.uint32) == gt[:, e].view(np.uint32)).all()
            else:                                                            # a similarity transform up to fp32 rounding of the result
                for s in range(t):
                    a, r, tr, _ = procrustes_fit(pred[s, e].astype(np.float64), gt[s, e].astype(np.float64))
                    assert abs(a / SCALE - 1.0) < 1e-5, (case.name, s, e, a)
                    resid = np.abs(a * pred[s, e].astype(np.float64) @ r + tr - gt[s, e]).max()
                    assert resid < 4 * 2.0 ** -24 * (np.abs(gt[s, e]).max() + np.abs(pred[s, e]).max()), (case.name, s, e, resid)
    if case.cls == "generic":                                                # det H is negative exactly in the mirrored envs
        for e in range(n):
            assert ((det[:, e] < 0) == (e in case.mirrored)).all(), (case.name, e, det[:, e])
    if case.cls == "slab":                                                   # across the slab the 4 cm of the prediction decide the sign of det H: both occur
        assert (det < 0).any() and (det > 0).any(), (case.name, det)
    return sv


# --------------------------------------------------------------------------- generators
def _rotation(rng):
    """A generic rotation (no axis of it near a coordinate axis), fp64."""
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _motion(rng, t, n, j):
    """A random body cloud per env moving smoothly, fp64 (T, N, J, 3)."""
    base = rng.standard_normal((n, j, 3)) * 0.3 + np.array([0.0, 0.0, 0.9])
    drift = rng.standard_normal((n, 1, 3)) * 0.05
    return np.stack([base + s * drift + 0.02 * rng.standard_normal((n, j, 3)) for s in range(t)])


def _perturbed(rng, gt, mirrored):
    """The prediction: the reference plus 4 cm per body and a 10 cm root offset; in ``mirrored`` envs its mirror image in x plus 4 cm."""
    t, n, j, _ = gt.shape
    pred = gt + 0.04 * rng.standard_normal((t, n, j, 3)) + 0.1 * rng.standard_normal((t, n, 1, 3))
    for e in mirrored:
        pred[:, e] = gt[:, e] * np.array([-1.0, 1.0, 1.0]) + 0.04 * rng.standard_normal((t, j, 3))
    return pred


def _f32(x):
    return np.ascontiguousarray(x.astype(np.float32))


def _flatten(x, e, axis):
    """Give every body of env e the coordinate of body 0, in place on the fp32 array: bit-identical over the bodies."""
    x[:, e, :, axis] = x[:, e, :1, axis]


def generic(j, n, seed, t=5, mirrored=None, tag=""):
    rng = np.random.default_rng(seed)
    mirrored = ((n - 1,) if n >= 2 else ()) if mirrored is None else tuple(mirrored)
    gt = _motion(rng, t, n, j)
    return Case(f"generic{tag}-j{j}-n{n}", "generic", _f32(_perturbed(rng, gt, mirrored)), _f32(gt), mirrored=mirrored)


def slab(j, n, seed, thickness, t=5):
    """thickness > 0: the reference's y is a constant plus ``thickness`` metres of noise.  thickness == 0: the reference is exactly planar in
    fp64, turned by a generic rotation, carried 20 and 30 m away from the origin and only then rounded to fp32, which leaves it about
    2^-24 of that distance (1e-6 m) thick."""
    rng = np.random.default_rng(seed)
    mirrored = (n - 1,)
    gt = _motion(rng, t, n, j)
    gt[..., 1] = gt[:, :, :1, 1] + thickness * rng.standard_normal((t, n, j))
    if thickness == 0.0:
        for e in range(n):
            c = gt[:, e].mean((0, 1))
            gt[:, e] = (gt[:, e] - c) @ _rotation(rng) + c + np.array([20.0, -30.0, 0.0])
    return Case(f"slab-j{j}-{thickness:g}", "slab", _f32(_perturbed(rng, _f32(gt).astype(np.float64), mirrored)), _f32(gt), mirrored=mirrored)


def gt_planar(j, n, seed, t=5):
    rng = np.random.default_rng(seed)
    mirrored = (n - 2,)
    gt = _f32(_motion(rng, t, n, j))
    axes = tuple((e + 1) % 3 for e in range(n))                              # y, z, x, y, z: every row of H is the zero one somewhere
    for e in range(n):
        _flatten(gt, e, axes[e])
    pred = _perturbed(rng, gt.astype(np.float64), ())
    for e in mirrored:                                                       # mirrored THROUGH its reference's plane: the fit has to turn it over
        m = np.ones(3)
        m[axes[e]] = -1.0
        pred[:, e] = gt[:, e] * m + 0.04 * rng.standard_normal((t, j, 3))
    return Case(f"gt_planar-j{j}", "gt_planar", _f32(pred), gt, mirrored=mirrored, gt_axis=axes)


def pred_planar(j, n, seed, t=5):
    rng = np.random.default_rng(seed)
    gt = _f32(_motion(rng, t, n, j))
    pred = _f32(_perturbed(rng, gt.astype(np.float64), ()))
    axes = tuple((e + 2) % 3 for e in range(n))
    for e in range(n):
        _flatten(pred, e, axes[e])
    return Case(f"pred_planar-j{j}", "pred_planar", pred, gt, pred_axis=axes)


def both_planar(j, n, seed, t=5):
    """Even envs: both clouds flat on the same axis (H has a zero row and the matching zero column); odd envs: on different axes, the
    prediction being the perturbed reference with those two coordinates exchanged (so the two planes still hold the same figure)."""
    rng = np.random.default_rng(seed)
    gt = _f32(_motion(rng, t, n, j))
    g_axes = tuple(e % 3 for e in range(n))
    p_axes = tuple((e + (e % 2)) % 3 for e in range(n))
    for e in range(n):
        _flatten(gt, e, g_axes[e])
    pred = _f32(_perturbed(rng, gt.astype(np.float64), ()))
    for e in range(n):
        if p_axes[e] != g_axes[e]:
            pred[:, e][..., [g_axes[e], p_axes[e]]] = pred[:, e][..., [p_axes[e], g_axes[e]]]
        _flatten(pred, e, p_axes[e])
    return Case(f"both_planar-j{j}", "both_planar", pred, gt, gt_axis=g_axes, pred_axis=p_axes)


def three_bodies(n, seed, t=5):
    rng = np.random.default_rng(seed)
    gt = _motion(rng, t, n, 3)
    return Case("three_bodies", "three_bodies", _f32(_perturbed(rng, gt, ())), _f32(gt))


def exact(j, n, seed, t=5, identical=(1, 4)):
    """``identical`` envs: pred bit-equal to gt.  The others: pred = (gt - shift) R^T / 1.7 in fp64, so that 1.7 pred R + shift gives gt back."""
    rng = np.random.default_rng(seed)
    gt = _f32(_motion(rng, t, n, j))
    pred = gt.astype(np.float64)
    for e in range(n):
        if e not in identical:
            r, shift = _rotation(rng), 0.3 * rng.standard_normal(3)
            pred[:, e] = (pred[:, e] - shift) @ r.T / SCALE
    return Case(f"exact-j{j}", "exact", _f32(pred), gt, identical=tuple(identical))


def one_body(n, seed, t=5):
    rng = np.random.default_rng(seed)
    gt = _motion(rng, t, n, 1)
    return Case(f"one_body-n{n}", "one_body", _f32(_perturbed(rng, gt, ())), _f32(gt))


def two_bodies(n, seed, t=5):
    rng = np.random.default_rng(seed)
    gt = _motion(rng, t, n, 2)
    return Case(f"two_bodies-n{n}", "two_bodies", _f32(_perturbed(rng, gt, ())), _f32(gt))


def gt_collinear(j, n, seed, t=5):
    """Even envs: the reference on a line along a coordinate axis (exactly collinear in fp32); odd envs: along a generic direction."""
    rng = np.random.default_rng(seed)
    gt = _motion(rng, t, n, j)
    for e in range(n):
        d = np.eye(3)[(e // 2) % 3] if e % 2 == 0 else _rotation(rng)[0]
        gt[:, e] = gt[:, e, :1] + (gt[:, e] @ d)[..., None] * d
    gt = _f32(gt)
    for e in range(0, n, 2):
        for k in range(3):
            if k != (e // 2) % 3:
                _flatten(gt, e, k)
    return Case(f"gt_collinear-j{j}", "gt_collinear", _f32(_perturbed(rng, gt.astype(np.float64), ())), gt)


def pred_point(j, n, seed, t=5):
    rng = np.random.default_rng(seed)
    gt = _f32(_motion(rng, t, n, j))
    pred = _f32(_perturbed(rng, gt.astype(np.float64), ()))
    pred[:] = pred[:, :, :1]
    return Case(f"pred_point-j{j}", "pred_point", np.ascontiguousarray(pred), gt)


def gt_point(j, n, seed, t=5):
    rng = np.random.default_rng(seed)
    gt = _f32(_motion(rng, t, n, j))
    pred = _f32(_perturbed(rng, gt.astype(np.float64), ()))
    gt[:] = gt[:, :, :1]
    return Case(f"gt_point-j{j}", "gt_point", pred, np.ascontiguousarray(gt))


# --------------------------------------------------------------------------- the cases the tests run
N = 5
SLAB_THICKNESS = (1e-3, 1e-5, 1e-6, 0.0)
# sigma3 of a slab's H changes sign with the prediction's noise, so it comes arbitrarily close to zero: seeds whose 25 fits all stay inside the class
SLAB_SEEDS = {24: (64, 65, 42, 40), 52: (92, 93, 46, 61)}
LANE_EDGES = tuple((j, n) for j in (4, 31, 32) for n in (1, 4, 5)) + tuple((j, n) for j in (33, 63, 64) for n in (1, 2, 3))


def rank_cases(cls):
    """The cases of a class for the rank tests: J = 24 and 52 (three_bodies: 3), N = 5."""
    if cls == "three_bodies":
        return [three_bodies(N, 37)]
    if cls == "slab":
        return [slab(j, N, SLAB_SEEDS[j][i], th) for j in (24, 52) for i, th in enumerate(SLAB_THICKNESS)]
    make = {"generic": generic, "gt_planar": gt_planar, "pred_planar": pred_planar, "both_planar": both_planar, "exact": exact}[cls]
    return [make(j, N, {"generic": 10, "gt_planar": 50, "pred_planar": 60, "both_planar": 70, "exact": 80}[cls] + j) for j in (24, 52)]


def unreferenced_cases(cls):
    if cls == "one_body":
        return [one_body(N, 91)]
    if cls == "two_bodies":
        return [two_bodies(N, 92)]
    make = {"gt_collinear": gt_collinear, "pred_point": pred_point, "gt_point": gt_point}[cls]
    return [make(j, N, 93 + j) for j in (24, 52)]


LANE_SEEDS_J4 = {1: 1341, 4: 1344, 5: 2345}      # four random bodies are often nearly coplanar: seeds whose every fit is in the class


def lane_case(j, n):
    return generic(j, n, LANE_SEEDS_J4[n] if j == 4 else 300 + 10 * j + n, tag="-lanes")


MASK_EDGES = (31, 64)                             # N = 9, every second env masked
STEP_EDGES = (24, 52)                             # the num_steps edges (N = 6, five steps) and the six-step sequences (N = 5)


def mask_case(j):
    return generic(j, 9, 500 + j, tag="-mask")


def num_steps_case(j):
    return generic(j, 6, 600 + j, tag="-numsteps")


def six_step_case(j):
    return generic(j, N, 700 + j, t=6, tag="-sixsteps")


def all_referenced_cases():
    return ([c for cls in REFERENCED for c in rank_cases(cls)] + [lane_case(j, n) for j, n in LANE_EDGES] + [mask_case(j) for j in MASK_EDGES] +
            [num_steps_case(j) for j in STEP_EDGES] + [six_step_case(j) for j in STEP_EDGES])


def all_cases():
    return all_referenced_cases() + [c for cls in UNREFERENCED for c in unreferenced_cases(cls)]
