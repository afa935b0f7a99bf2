"""The evaluation metrics of include/pulse_hip.h section 2b'' restated in fp64 numpy: the yardstick of the accumulation kernel
(tests/test_eval_metrics_gpu.py) and of the sweep's eight numbers (tests/test_eval_sweep_gpu.py).  Not a test module."""
import numpy as np


def procrustes_fit(pred, gt):
    """The similarity Procrustes fit of the common p_mpjpe (predicted aligned onto target) for one frame: pred, gt (J, 3) float64.
    Returns (a, r, t, H): a * pred @ r + t is the aligned prediction.  LAPACK returns full orthonormal U and V whatever the rank of H,
    so r is a rotation also where H has a zero singular value (tests/test_eval_metrics_edges_cpu.py)."""
    mu_x, mu_y = gt.mean(0, keepdims=True), pred.mean(0, keepdims=True)
    x0, y0 = gt - mu_x, pred - mu_y
    norm_x, norm_y = np.sqrt((x0 ** 2).sum()), np.sqrt((y0 ** 2).sum())
    x0, y0 = x0 / norm_x, y0 / norm_y
    h = x0.T @ y0
    u, s, vt = np.linalg.svd(h)
    v = vt.T
    r = v @ u.T
    if np.linalg.det(r) < 0:
        v[:, -1] *= -1
        s[-1] *= -1
        r = v @ u.T
    a = s.sum() * norm_x / norm_y
    t = mu_x - a * mu_y @ r
    return a, r, t, h


def procrustes(pred, gt):
    """The aligned prediction of procrustes_fit and H (for the conditioning check)."""
    a, r, t, h = procrustes_fit(pred, gt)
    return a * pred @ r + t, h


def step_terms(pred, gt, pa=True):
    """pred, gt (T, J, 3) float64 -> dict of per-frame terms in mm: mpjpe_g / mpjpe_l / mpjpe_pa (T,), vel_dist (T - 1,), accel_dist (T - 2,).
    pa=False leaves the fit out (mpjpe_pa is NaN): for clouds on which it divides 0 / 0 or its rotation is arbitrary."""
    t = pred.shape[0]
    out = {"mpjpe_g": np.linalg.norm(pred - gt, axis=-1).mean(-1) * 1000.0}
    pl, gl = pred - pred[:, :1], gt - gt[:, :1]
    out["mpjpe_l"] = np.linalg.norm(pl - gl, axis=-1).mean(-1) * 1000.0
    if pa:
        out["mpjpe_pa"] = np.array([np.linalg.norm(procrustes(pl[i], gl[i])[0] - gl[i], axis=-1).mean() for i in range(t)]).reshape(t) * 1000.0
    else:
        out["mpjpe_pa"] = np.full(t, np.nan)
    dv = (pred[1:] - pred[:-1]) - (gt[1:] - gt[:-1]) if t >= 2 else np.zeros((0,) + pred.shape[1:])
    da = (pred[2:] - 2 * pred[1:-1] + pred[:-2]) - (gt[2:] - 2 * gt[1:-1] + gt[:-2]) if t >= 3 else np.zeros((0,) + pred.shape[1:])
    out["vel_dist"] = np.linalg.norm(dv, axis=-1).mean(-1) * 1000.0
    out["accel_dist"] = np.linalg.norm(da, axis=-1).mean(-1) * 1000.0
    return out


def accumulator_row(pred, gt, pa=True):
    """The (8,) row the kernel holds after the counted frames pred / gt (T, J, 3) of one env: five sums and three frame counts."""
    m = step_terms(np.asarray(pred, np.float64), np.asarray(gt, np.float64), pa)
    return np.array([m["mpjpe_g"].sum(), m["mpjpe_l"].sum(), m["mpjpe_pa"].sum(), m["vel_dist"].sum(), m["accel_dist"].sum(),
                     len(m["mpjpe_g"]), len(m["vel_dist"]), len(m["accel_dist"])], dtype=np.float64)


def eval_info(pred_all, gt_all, failed):
    """The reference's eight numbers (im_amp.py:314-341) from per-motion (T_i, J, 3) arrays: every metric is the mean over the concatenated
    frames of the motions it covers ("all" / the successful ones; "succ" falls back to "all" when nothing succeeded)."""
    rows = np.stack([accumulator_row(p, g) for p, g in zip(pred_all, gt_all)])
    failed = np.asarray(failed, bool)

    def means(r):
        s = r.sum(0)
        return {"mpjpe_g": s[0] / s[5], "mpjpe_l": s[1] / s[5], "mpjpe_pa": s[2] / s[5], "vel_dist": s[3] / s[6], "accel_dist": s[4] / s[7]}
    all_ = means(rows)
    succ = means(rows[~failed]) if (~failed).any() else all_
    return {"eval_success_rate": 1.0 - failed.mean(), "eval_mpjpe_all": all_["mpjpe_g"], "eval_mpjpe_succ": succ["mpjpe_g"],
            "accel_dist": succ["accel_dist"], "vel_dist": succ["vel_dist"], "mpjpel_all": all_["mpjpe_l"], "mpjpel_succ": succ["mpjpe_l"],
            "mpjpe_pa": succ["mpjpe_pa"]}
