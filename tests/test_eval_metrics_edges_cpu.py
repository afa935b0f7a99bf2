"""CPU: the yardstick of tests/test_eval_metrics_edges_gpu.py where its SVD completion matters.  On every referenced class of
tests/eval_metrics_cases.py the fp64 restatement's fit is a rotation and a minimum of the aligned error also where H has a zero singular
value, and every generated case is what its class says."""
import numpy as np
import pytest

from tests import eval_metrics_cases as cases
from tests.eval_metrics_ref import procrustes_fit

ALL = cases.all_cases()
REFERENCED = cases.all_referenced_cases()


def _frames(case):
    """(s, e, root-relative pred, root-relative gt) in fp64, as step_terms hands them to the fit."""
    p, g = case.pred.astype(np.float64), case.gt.astype(np.float64)
    for s in range(p.shape[0]):
        for e in range(p.shape[1]):
            yield s, e, p[s, e] - p[s, e, :1], g[s, e] - g[s, e, :1]


def _axis_rotation(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, k = (axis + 1) % 3, (axis + 2) % 3
    r = np.eye(3)
    r[i, i], r[i, k], r[k, i], r[k, k] = c, -s, s, c
    return r


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_class_conditions_hold(case):
    case.conditions()


def test_every_class_is_generated():
    assert {c.cls for c in ALL} == set(cases.REFERENCED) | set(cases.UNREFERENCED)
    assert {c.cls for c in REFERENCED} == set(cases.REFERENCED)
    assert {(c.pred.shape[2], c.pred.shape[1]) for c in ALL if c.cls == "generic"} == set(cases.LANE_EDGES) | {(24, 5), (52, 5), (31, 9), (64, 9), (24, 6), (52, 6)}
    assert all(c.pred.shape[0] <= 6 and c.pred.shape[1] <= 9 and c.pred.shape[2] <= 64 for c in ALL)


@pytest.mark.parametrize("case", REFERENCED, ids=lambda c: c.name)
def test_restatement_returns_a_rotation(case):
    for s, e, pl, gl in _frames(case):
        _, r, _, _ = procrustes_fit(pl, gl)
        assert np.abs(r @ r.T - np.eye(3)).max() <= 1e-12, (s, e)
        assert abs(np.linalg.det(r) - 1.0) <= 1e-12, (s, e, np.linalg.det(r))


@pytest.mark.parametrize("case", REFERENCED, ids=lambda c: c.name)
def test_restatement_is_a_minimum_over_rotations(case):
    """First-order optimality: with scale and shift refitted in closed form, turning r by a small angle about any axis, either way, never
    lowers the summed squared error by more than 1e-12 of itself -- plus what rounding does to a sum of squared differences of numbers
    of the cloud's size |X0|: each difference carries a few eps |X0|, so the sum moves by about 8 eps sqrt(sse) |X0| + 64 eps^2 |X0|^2
    (in the "exact" class the error itself is ~ 0 and this is all there is)."""
    eps = np.finfo(np.float64).eps
    for s, e, pl, gl in _frames(case):
        a, r, t, _ = procrustes_fit(pl, gl)
        x0 = gl - gl.mean(0)
        sx = (x0 ** 2).sum()

        def sse(rot):                                                        # the best similarity fit that uses rotation ``rot``
            y = (pl - pl.mean(0)) @ rot
            return ((np.sum(x0 * y) / np.sum(y * y) * y - x0) ** 2).sum()
        base = ((a * pl @ r + t - gl) ** 2).sum()
        slack = 1e-12 * base + 8 * eps * np.sqrt(base * sx) + 64 * eps ** 2 * sx
        assert abs(base - sse(r)) <= slack, (s, e, base, sse(r))             # the returned a and t are the closed-form ones for r
        for axis in range(3):
            for angle in (1e-4, -1e-4, 1e-2, -1e-2):
                assert sse(r @ _axis_rotation(axis, angle)) >= base - slack, (s, e, axis, angle)
