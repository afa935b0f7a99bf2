"""GPU: pulse_im_eval_accum (include/pulse_hip.h section 2b'') against the fp64 numpy restatement of its five per-frame terms
(tests/eval_metrics_ref.py).  The kernel and numpy see the same fp32 inputs and both work in fp64; they differ in the order of the sums
and in the SVD algorithm (fixed-sweep Jacobi against LAPACK), so every accumulator entry is held to 1e-9 relative + 1e-9 mm and the
frame counts exactly."""
import numpy as np
import pytest
import torch

from pulse_amd import ops
from tests.eval_metrics_ref import accumulator_row, procrustes

pytestmark = pytest.mark.gpu

N, STEPS = 5, 5                                   # 5 envs: a partial last workgroup at 4 (32-lane groups) and at 2 (64-lane groups) envs per workgroup
NUM_STEPS = [1, 2, 3, 4, 9]                       # counted frames 0 / 1 / 2 / 3 / 5: velocity frames 0 / 0 / 1 / 2 / 4, acceleration frames 0 / 0 / 0 / 1 / 3
MIRRORED = 3                                      # this env's prediction is a mirror image of its reference: det R < 0


def _data(j, seed):
    """(pred, gt) (STEPS, N, J, 3) float32: a random body cloud per env moving smoothly, the prediction a perturbed copy."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(N, j, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 0.9])
    drift = torch.randn(N, 1, 3, generator=g) * 0.05
    gt = torch.stack([base + s * drift + 0.02 * torch.randn(N, j, 3, generator=g) for s in range(STEPS)])
    pred = gt + 0.04 * torch.randn(STEPS, N, j, 3, generator=g) + 0.1 * torch.randn(STEPS, N, 1, 3, generator=g)
    mirrored = gt[:, MIRRORED] * torch.tensor([-1.0, 1.0, 1.0]) + 0.01 * torch.randn(STEPS, j, 3, generator=g)
    pred[:, MIRRORED] = mirrored
    return pred.float().contiguous(), gt.float().contiguous()


def _check_conditioning(pred, gt):
    """Every H of the fit has its smallest singular value >= 1e-3 of its largest (and the mirrored env takes the reflection branch)."""
    p, g = pred.double().numpy(), gt.double().numpy()
    for s in range(STEPS):
        for e in range(N):
            _, h = procrustes(p[s, e] - p[s, e, :1], g[s, e] - g[s, e, :1])
            sv = np.linalg.svd(h, compute_uv=False)
            assert sv[-1] >= 1e-3 * sv[0], (s, e, sv)
            assert (np.linalg.det(h) < 0) == (e == MIRRORED), (s, e)


def _expected(pred, gt, num_steps=NUM_STEPS):
    p, g = pred.double().numpy(), gt.double().numpy()
    return np.stack([accumulator_row(p[:max(min(STEPS, ns - 1), 0), e], g[:max(min(STEPS, ns - 1), 0), e]) for e, ns in enumerate(num_steps)])


def _pitched(dev, j):
    """Device buffers whose rows are wider than what the kernel uses; the padding is poisoned."""
    rb = torch.full((N, 13 * j + 7), float("nan"), device=dev)
    ref = torch.full((N, 3 * j + 5), float("nan"), device=dev)
    acc = torch.full((N, 11), -7.0, dtype=torch.float64, device=dev)
    acc[:, :8] = 0.0
    ring = torch.full((N, 2, 2, j, 3), float("nan"), device=dev)            # the ring needs no initialisation
    return rb, ref, acc, ring


def _load(rb, ref, pred_s, gt_s, j):
    v = rb[:, :13 * j].view(N, j, 13)
    v.fill_(123.0)                                                          # rotations / velocities: never read
    v[..., 0:3] = pred_s.to(rb.device)
    r = ref[:, :3 * j].view(N, j, 3)
    r.copy_(gt_s.to(ref.device))
    return v, r


def _assert_rows(got, want, rows=range(N)):
    for e in rows:
        print(f"env {e}: got {got[e].tolist()} want {want[e].tolist()}")
    for e in rows:
        assert np.array_equal(got[e, 5:], want[e, 5:]), (e, got[e, 5:], want[e, 5:])
        err = np.abs(got[e, :5] - want[e, :5])
        assert (err <= 1e-9 * np.abs(want[e, :5]) + 1e-9).all(), (e, err, want[e, :5])


@pytest.mark.parametrize("j", [24, 52])
def test_accumulator_matches_numpy(dev, j):
    pred, gt = _data(j, 100 + j)
    _check_conditioning(pred, gt)
    want = _expected(pred, gt)
    assert want[:, 5].tolist() == [0, 1, 2, 3, 5] and want[:, 6].tolist() == [0, 0, 1, 2, 4] and want[:, 7].tolist() == [0, 0, 0, 1, 3]
    rb, ref, acc, ring = _pitched(dev, j)
    num_steps = torch.tensor(NUM_STEPS, dtype=torch.int32, device=dev)
    for s in range(STEPS):
        v, r = _load(rb, ref, pred[s], gt[s], j)
        ops.im_eval_accum(v, r, num_steps, s, ring, acc[:, :8])
    torch.cuda.synchronize()
    got = acc.cpu().numpy()
    assert (got[:, 8:] == -7.0).all(), "the kernel wrote past the 8 doubles of a row"
    assert np.isfinite(got).all()
    _assert_rows(got[:, :8], want)
    # the ring holds the last two steps, bit for bit
    ring_c = ring.cpu()
    for s in (STEPS - 2, STEPS - 1):
        assert torch.equal(ring_c[:, s & 1, 0], pred[s]) and torch.equal(ring_c[:, s & 1, 1], gt[s])


@pytest.mark.parametrize("j", [24, 52])
def test_mask_and_restart_carry_the_state(dev, j):
    """The same sweep as two launch sequences over different buffers, one env masked out throughout and one env's prediction jumping back
    onto its reference in the middle (a mid-batch restart): the masked env's row and ring stay as they were, every other env's sums and
    counts carry on across the sequences and the jump counts like any other step."""
    pred, gt = _data(j, 200 + j)
    pred[3:, 4] = gt[3:, 4] + 0.001                                         # env 4 restarts at step 3
    _check_conditioning(pred, gt)
    want = _expected(pred, gt)
    masked = 1
    mask = torch.ones(N, dtype=torch.bool, device=dev)
    mask[masked] = False
    num_steps = torch.tensor(NUM_STEPS, dtype=torch.int32, device=dev)
    _, _, acc, ring = _pitched(dev, j)
    acc[masked, :8] = 5.5
    for first, last in ((0, 3), (3, STEPS)):
        rb, ref, _, _ = _pitched(dev, j)                                    # fresh input buffers per sequence
        for s in range(first, last):
            v, r = _load(rb, ref, pred[s], gt[s], j)
            ops.im_eval_accum(v, r, num_steps, s, ring, acc[:, :8], env_mask=mask)
    torch.cuda.synchronize()
    got = acc.cpu().numpy()[:, :8]
    assert (got[masked] == 5.5).all() and torch.isnan(ring[masked]).all()
    _assert_rows(got, want, rows=[e for e in range(N) if e != masked])


def test_wrapper_rejects_bad_tensors(dev):
    j = 24
    ring, acc = ops.im_eval_state(N, j, dev)
    rb, ref = torch.zeros(N, j, 13, device=dev), torch.zeros(N, j, 3, device=dev)
    ns = torch.full((N,), 4, dtype=torch.int32, device=dev)
    ops.im_eval_accum(rb, ref, ns, 0, ring, acc)
    with pytest.raises(ValueError, match="GPU"):
        ops.im_eval_accum(rb.cpu(), ref, ns, 0, ring, acc)
    with pytest.raises(TypeError, match="dtype"):
        ops.im_eval_accum(rb, ref, ns.long(), 0, ring, acc)
    with pytest.raises(TypeError, match="dtype"):
        ops.im_eval_accum(rb, ref, ns, 0, ring, acc.float())
    with pytest.raises(ValueError, match="ref_pos"):
        ops.im_eval_accum(rb, ref[:, :20], ns, 0, ring, acc)
    with pytest.raises(ValueError, match="contiguous"):
        ops.im_eval_accum(torch.zeros(N, j, 26, device=dev)[..., ::2], ref, ns, 0, ring, acc)
    with pytest.raises(ValueError, match="ring"):
        ops.im_eval_accum(rb, ref, ns, 0, ring[:, :1], acc)
