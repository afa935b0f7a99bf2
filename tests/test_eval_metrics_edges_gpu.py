"""GPU: pulse_im_eval_accum (include/pulse_hip.h section 2b'') where tests/test_eval_metrics_gpu.py does not look: a Procrustes fit whose H has
a small or a zero singular value, body counts at the edges of the 32- and 64-lane groups, and num_steps / step-parity edges.  The cases
and their classes come from tests/eval_metrics_cases.py (each test re-checks the class on the arrays it runs), the yardstick is the fp64
numpy restatement (tests/eval_metrics_ref.py; tests/test_eval_metrics_edges_cpu.py holds it to account on the same cases).  The bound is
that suite's: 1e-9 relative + 1e-9 mm per accumulator entry, frame counts exact.  Classes without a reference (the restatement divides
0 / 0 or its rotation is arbitrary) are held to it in columns 0, 1, 3, 4 and the counts, and their Procrustes sum to finite and >= 0.

Every buffer is pitched and poisoned as in that suite: NaN row padding, a NaN ring, accumulator columns 8 and up that must stay as they were.
Each test prints its largest error as a fraction of the bound (profiles/eval_metrics_edges.txt: python -m pytest <this file> -m gpu -s -q)."""
import numpy as np
import pytest
import torch

from pulse_amd import ops
from tests import eval_metrics_cases as cases
from tests.eval_metrics_ref import accumulator_row, step_terms

pytestmark = pytest.mark.gpu

REL, ABS = 1e-9, 1e-9                             # per accumulator entry, mm
NUM_STEPS = [1, 2, 3, 4, 9]                       # counted frames 0 / 1 / 2 / 3 / 5 of five steps
INT32_MAX = 2 ** 31 - 1


# --------------------------------------------------------------------------- the yardstick
def _counted(ns, steps):
    return [s for s in steps if s < ns - 1]


def _expected(case, num_steps, steps):
    """(N, 8) rows after launching ``steps`` (consecutive step indices; the ring holds the steps before them).  From step 0 this is
    accumulator_row over the counted frames; from a later step, the same per-frame terms summed over the counted steps.  Without a
    reference the Procrustes column is NaN."""
    pa = case.cls in cases.REFERENCED
    p, g = case.pred.astype(np.float64), case.gt.astype(np.float64)
    rows = []
    for e, ns in enumerate(num_steps):
        cnt = _counted(ns, steps)
        if steps[0] == 0:
            rows.append(accumulator_row(p[:len(cnt), e], g[:len(cnt), e], pa))
            continue
        m = step_terms(p[:, e], g[:, e], pa)
        vel, acc = [s for s in cnt if s >= 1], [s for s in cnt if s >= 2]
        rows.append(np.array([sum(m["mpjpe_g"][s] for s in cnt), sum(m["mpjpe_l"][s] for s in cnt), sum(m["mpjpe_pa"][s] for s in cnt),
                              sum(m["vel_dist"][s - 1] for s in vel), sum(m["accel_dist"][s - 2] for s in acc), len(cnt), len(vel), len(acc)], dtype=np.float64))
    return np.stack(rows)


def _assert_rows(case, got, want, rows=None, what=""):
    """Counts exact, sums within REL * |want| + ABS; the Procrustes column of a class without a reference only finite and >= 0."""
    rows = range(got.shape[0]) if rows is None else rows
    cols = [0, 1, 2, 3, 4] if case.cls in cases.REFERENCED else [0, 1, 3, 4]
    worst = 0.0
    for e in rows:
        err = np.abs(got[e, cols] - want[e, cols]) / (REL * np.abs(want[e, cols]) + ABS)
        worst = max(worst, err.max())
        print(f"  {case.name}{what} env {e}: got {got[e].tolist()} want {want[e].tolist()} err/bound {err.tolist()}")
    print(f"EDGES class={case.cls} case={case.name}{what} worst_err_over_bound={worst:.3e}")
    assert np.isfinite(got).all(), got
    for e in rows:
        assert np.array_equal(got[e, 5:], want[e, 5:]), (e, got[e, 5:], want[e, 5:])
        assert got[e, 2] >= 0.0, (e, got[e, 2])
        err = np.abs(got[e, cols] - want[e, cols])
        assert (err <= REL * np.abs(want[e, cols]) + ABS).all(), (case.name, e, err, want[e, cols])


# --------------------------------------------------------------------------- buffers and launches
class Buffers:
    """Device buffers whose rows are wider than what the kernel uses, padding poisoned; the ring needs no initialisation."""

    def __init__(self, dev, n, j):
        self.n, self.j = n, j
        self.rb = torch.full((n, 13 * j + 7), float("nan"), device=dev)
        self.ref = torch.full((n, 3 * j + 5), float("nan"), device=dev)
        self.acc = torch.full((n, 11), -7.0, dtype=torch.float64, device=dev)
        self.acc[:, :8] = 0.0
        self.ring = torch.full((n, 2, 2, j, 3), float("nan"), device=dev)

    def launch(self, case, s, num_steps, mask=None):
        n, j = self.n, self.j
        v = self.rb[:, :13 * j].view(n, j, 13)
        v.fill_(123.0)                                                      # rotations / velocities: never read
        v[..., 0:3] = torch.from_numpy(case.pred[s]).to(v.device)
        r = self.ref[:, :3 * j].view(n, j, 3)
        r.copy_(torch.from_numpy(case.gt[s]).to(r.device))
        ops.im_eval_accum(v, r, num_steps, s, self.ring, self.acc[:, :8], env_mask=mask)

    def rows(self):
        """The (N, 8) accumulator rows; everything around them must be as it was."""
        torch.cuda.synchronize()
        got = self.acc.cpu().numpy()
        assert (got[:, 8:] == -7.0).all(), "the kernel wrote past the 8 doubles of a row"
        assert torch.isnan(self.rb[:, 13 * self.j:]).all() and torch.isnan(self.ref[:, 3 * self.j:]).all()
        return got[:, :8]

    def assert_ring_holds(self, case, last, envs=None):
        """Slot s & 1 holds step s for the last two steps launched, bit for bit."""
        ring = self.ring.cpu().numpy().view(np.uint32)
        envs = range(self.n) if envs is None else envs
        for s in (last - 1, last):
            if s < 0:
                continue
            for e in envs:
                assert np.array_equal(ring[e, s & 1, 0], case.pred[s, e].view(np.uint32)), (s, e)
                assert np.array_equal(ring[e, s & 1, 1], case.gt[s, e].view(np.uint32)), (s, e)


def _run(dev, case, num_steps, steps=None):
    """Launch ``steps`` (default: every step of the case, from 0) on fresh buffers and return them with the expected rows."""
    case.conditions()
    t, n, j = case.pred.shape[:3]
    steps = list(range(t)) if steps is None else steps
    assert len(num_steps) == n
    buf = Buffers(dev, n, j)
    ns = torch.tensor(num_steps, dtype=torch.int32, device=dev)
    for s in steps:
        buf.launch(case, s, ns)
    return buf, _expected(case, num_steps, steps)


# --------------------------------------------------------------------------- 1. rank classes
@pytest.mark.parametrize("cls", cases.REFERENCED)
def test_rank_class_matches_numpy(dev, cls):
    """J = 24 and 52 (three_bodies: 3), N = 5 with num_steps 1 / 2 / 3 / 4 / 9, so the velocity and acceleration paths run beside the fit."""
    for case in cases.rank_cases(cls):
        assert case.cls == cls
        buf, want = _run(dev, case, NUM_STEPS)
        assert want[:, 5].tolist() == [0, 1, 2, 3, 5] and want[:, 6].tolist() == [0, 0, 1, 2, 4] and want[:, 7].tolist() == [0, 0, 0, 1, 3]
        got = buf.rows()
        _assert_rows(case, got, want)
        buf.assert_ring_holds(case, case.pred.shape[0] - 1)
        for e in case.identical:                                            # pred bit-equal to gt: every term is zero, the fit's to rounding
            print(f"  {case.name} identical env {e}: Procrustes sum {got[e, 2]:.3e} mm over {int(got[e, 5])} frames")
            assert got[e, 5] >= 1 and got[e, 2] <= 1e-9 * got[e, 5], (e, got[e])
            assert (got[e, [0, 1, 3, 4]] == 0.0).all(), (e, got[e])


@pytest.mark.parametrize("cls", cases.UNREFERENCED)
def test_class_without_reference_stays_finite(dev, cls):
    for case in cases.unreferenced_cases(cls):
        assert case.cls == cls
        buf, want = _run(dev, case, NUM_STEPS)
        _assert_rows(case, buf.rows(), want)
        buf.assert_ring_holds(case, case.pred.shape[0] - 1)


# --------------------------------------------------------------------------- 2. lane edges
def _lane_num_steps(n):
    return [9, 4, 3, 2, 1][:n]


@pytest.mark.parametrize("j,n", cases.LANE_EDGES)
def test_lane_edges_match_numpy(dev, j, n):
    """Bodies up to, at and past the 32-lane group, and the same for the 64-lane one; envs that fill a workgroup (4 / 2), leave it partly
    empty (1) and spill into a second (5 / 3).  Lanes J .. LB - 1 must feed exact zeros into every butterfly."""
    case = cases.lane_case(j, n)
    assert case.pred.shape[1:3] == (n, j)
    buf, want = _run(dev, case, _lane_num_steps(n))
    assert want[0, 5:].tolist() == [5, 4, 3]
    _assert_rows(case, buf.rows(), want)
    buf.assert_ring_holds(case, 4)


@pytest.mark.parametrize("j,n", [(j, n) for j in (1, 2) for n in (1, 4, 5)])
def test_one_and_two_bodies(dev, j, n):
    case = (cases.one_body if j == 1 else cases.two_bodies)(n, 800 + 10 * j + n)
    buf, want = _run(dev, case, _lane_num_steps(n))
    got = buf.rows()
    _assert_rows(case, got, want)
    if j == 1:                                                              # root-relative, one body is the origin: nothing to align
        assert (got[:, 1:3] == 0.0).all()
    buf.assert_ring_holds(case, 4)


@pytest.mark.parametrize("j", cases.MASK_EDGES)
def test_every_second_env_masked(dev, j):
    """N = 9 (three workgroups of 32-lane groups, five of 64-lane ones), odd envs masked: their accumulator rows and rings keep every bit
    they held (random bit patterns, NaNs among them), the others match numpy."""
    case = cases.mask_case(j)
    case.conditions()
    n = 9
    num_steps = [9, 1, 2, 9, 3, 9, 4, 2, 9]
    masked = list(range(1, n, 2))
    live = [e for e in range(n) if e not in masked]
    mask = torch.ones(n, dtype=torch.bool, device=dev)
    mask[masked] = False
    buf = Buffers(dev, n, j)
    g = torch.Generator().manual_seed(j)
    held = torch.randint(-2 ** 31, 2 ** 31 - 1, (n, 2, 2, j, 3), generator=g, dtype=torch.int64).to(torch.int32)
    buf.ring.view(torch.int32)[masked] = held[masked].to(dev)
    buf.acc[masked, :8] = 5.5
    ns = torch.tensor(num_steps, dtype=torch.int32, device=dev)
    for s in range(5):
        buf.launch(case, s, ns, mask=mask)
    got = buf.rows()
    assert (got[masked] == 5.5).all()
    assert torch.equal(buf.ring.view(torch.int32)[masked].cpu(), held[masked])
    _assert_rows(case, got, _expected(case, num_steps, list(range(5))), rows=live)
    buf.assert_ring_holds(case, 4, envs=live)


# --------------------------------------------------------------------------- 3. step edges
@pytest.mark.parametrize("j", cases.STEP_EDGES)
def test_num_steps_edges(dev, j):
    """num_steps -1, 0 and 1 count no frame, 2 counts step 0, 3 steps 0 and 1, INT32_MAX every step.  A row that counts nothing stays
    all-zero (not merely small) while its ring is rewritten like any other."""
    case = cases.num_steps_case(j)
    num_steps = [-1, 0, 1, 2, 3, INT32_MAX]
    buf, want = _run(dev, case, num_steps)
    assert want[:, 5].tolist() == [0, 0, 0, 1, 2, 5] and want[:, 6].tolist() == [0, 0, 0, 0, 1, 4] and want[:, 7].tolist() == [0, 0, 0, 0, 0, 3]
    got = buf.rows()
    assert (got[:3].view(np.uint64) == 0).all(), got[:3]                    # + 0.0 in every entry
    _assert_rows(case, got, want)
    buf.assert_ring_holds(case, 4)


@pytest.mark.parametrize("j", cases.STEP_EDGES)
@pytest.mark.parametrize("start", [1, 3])
def test_sequence_starts_at_an_odd_step(dev, j, start):
    """A launch sequence whose first step index is odd, on a ring the host filled: slot 0 with step start - 1, slot 1 with step start - 2
    (start 1: with nothing, it stays NaN -- the acceleration term reads it and must not count it).  The sums are those of the counted
    steps alone, their differences reaching back into the ring."""
    case = cases.six_step_case(j)
    case.conditions()
    num_steps = [9, 9, 6, 5, 3]                                             # counted steps: < 8, < 8, < 5, < 4, < 2
    steps = list(range(start, 6))
    buf = Buffers(dev, cases.N, j)
    for s in (start - 2, start - 1):
        if s >= 0:
            buf.ring[:, s & 1, 0] = torch.from_numpy(case.pred[s]).to(dev)
            buf.ring[:, s & 1, 1] = torch.from_numpy(case.gt[s]).to(dev)
    ns = torch.tensor(num_steps, dtype=torch.int32, device=dev)
    for s in steps:
        buf.launch(case, s, ns)
    want = _expected(case, num_steps, steps)
    assert want[:, 5].tolist() == [6 - start, 6 - start, max(5 - start, 0), max(4 - start, 0), max(2 - start, 0)]
    assert want[0, 6] == 6 - start and want[0, 7] == 6 - max(start, 2)
    _assert_rows(case, buf.rows(), want, what=f"-from{start}")
    buf.assert_ring_holds(case, 5)


@pytest.mark.parametrize("j", cases.STEP_EDGES)
def test_six_steps_on_one_ring(dev, j):
    """Six steps, the ring's parity alternating three times, read back and compared after every one of them."""
    case = cases.six_step_case(j)
    case.conditions()
    num_steps = [9, 7, 6, 4, 2]
    buf = Buffers(dev, cases.N, j)
    ns = torch.tensor(num_steps, dtype=torch.int32, device=dev)
    for s in range(6):
        buf.launch(case, s, ns)
        _assert_rows(case, buf.rows(), _expected(case, num_steps, list(range(s + 1))), what=f"-after{s}")
        buf.assert_ring_holds(case, s)
