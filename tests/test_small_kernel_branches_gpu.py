"""GPU: the branches of the small rollout / update kernels that no other test launches -- partial chunks, scalar tails, capped grids,
uneven lane loops, optional outputs, workgroups without work -- each against a plain fp64 model written here (or the CPU oracle where named).

Every buffer a kernel writes is a view into a larger one filled with poison (NaN; 0xA5 for byte flags) in its pad columns and past its end,
and every test asserts that the poison is still there.  Every family prints its worst error as a fraction of its bound
(profiles/small_kernel_branches.txt records them).
"""
import math

import numpy as np
import pytest
import torch

from oracle import env_oracle as E
from pulse_amd import kernels as K, ops
from pulse_amd._lib import PulseLibraryError
from tests.rollout_record_ref import RolloutReference
from tests.test_env_kernels_gpu import ATOL

pytestmark = pytest.mark.gpu

NAN = float("nan")
FLAG = 0xA5                    # poison of byte buffers (flags are 0 / 1)
U24 = 2.0 ** -24               # one fp32 rounding, relative


# ------------------------------------------------------------------ bookkeeping: worst error / bound per family
_WORST = {}


def within(family, got, want, atol=0.0, rtol=0.0, bound=None):
    """|got - want| <= atol + rtol |want| (or the elementwise ``bound``) for every element, nothing masked; the family's worst ratio is kept."""
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    want = want.detach().cpu().double().numpy() if isinstance(want, torch.Tensor) else np.asarray(want, np.float64)
    assert got.shape == want.shape, (family, got.shape, want.shape)
    assert np.isfinite(want).all(), family
    assert np.isfinite(got).all(), f"{family}: non-finite output"
    err = np.abs(got - want)
    lim = (atol + rtol * np.abs(want)) if bound is None else np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    exact = lim == 0
    assert (err[exact] == 0).all(), f"{family}: error where the bound is zero"
    ratio = float((err[~exact] / lim[~exact]).max()) if (~exact).any() else 0.0
    _WORST[family] = max(_WORST.get(family, 0.0), ratio)
    assert ratio <= 1.0, f"{family}: worst error {ratio:.3f} x its bound (max |err| {err.max():.3e})"


def report(*families):
    for f in families:
        print(f"[small_kernel_branches] {f}: worst error / bound = {_WORST.get(f, 0.0):.3e}")


# ------------------------------------------------------------------ poisoned buffers
class Pitched:
    """A (rows, cols) matrix with row pitch ``pitch`` inside a flat poisoned buffer: ``lead`` elements in front, ``tail`` behind."""

    def __init__(self, rows, cols, pitch, dev, data=None, lead=0, tail=8, dtype=torch.float32, poison=NAN):
        assert pitch >= cols
        self.rows, self.cols, self.pitch, self.lead, self.poison = rows, cols, pitch, lead, poison
        self.flat = torch.full((lead + rows * pitch + tail,), poison, dtype=dtype, device=dev)
        self.full = self.flat[lead: lead + rows * pitch].view(rows, pitch)
        self.view = self.full[:, :cols]
        if data is not None:
            self.view.copy_(data.to(dev))

    def assert_poison(self, written_cols=None):
        """Everything outside columns [0, written_cols) of the rows is still poison."""
        w = self.cols if written_cols is None else written_cols
        out = torch.ones(self.flat.shape, dtype=torch.bool, device=self.flat.device)
        out[self.lead: self.lead + self.rows * self.pitch].view(self.rows, self.pitch)[:, :w] = False
        rest = self.flat[out]
        ok = torch.isnan(rest) if isinstance(self.poison, float) and math.isnan(self.poison) else rest == self.poison
        assert bool(ok.all()), "a kernel wrote outside its columns"


def flat(n, dev, data=None, tail=5, dtype=torch.float32, poison=NAN):
    """(buffer, view of its first n elements); the tail keeps the poison."""
    buf = torch.full((n + tail,), poison, dtype=dtype, device=dev)
    if data is not None:
        buf[:n] = data.to(dev)
    return buf, buf[:n]


def tail_intact(buf, n, poison=NAN):
    rest = buf[n:]
    return bool((torch.isnan(rest) if isinstance(poison, float) and math.isnan(poison) else rest == poison).all())


# ================================================================== 1. GAE
GAMMA, TAU = 0.99, 0.95


def _gae64(d, v, r, nv):
    """The recurrence of common_agent.py:493-505 in fp64.  (T, N) arrays."""
    adv, last = np.zeros_like(r), np.zeros(r.shape[1])
    for t in reversed(range(r.shape[0])):
        delta = r[t] + GAMMA * nv[t] - v[t]
        last = delta + GAMMA * TAU * (1.0 - d[t]) * last
        adv[t] = last
    return adv


def _done_sets(t, n, g):
    """Random dones at p = 0.2 with three special envs (all steps done / done at t = 0 only / done at t = T - 1 only) at the first, middle and
    last env; with fewer than three envs every special pattern gets a matrix of its own."""
    rand = (torch.rand(t, n, generator=g) < 0.2).to(torch.uint8)
    special = [torch.ones(t, dtype=torch.uint8), torch.zeros(t, dtype=torch.uint8), torch.zeros(t, dtype=torch.uint8)]
    special[1][0] = 1
    special[2][t - 1] = 1
    if n >= 3:
        for col, s in zip((0, n // 2, n - 1), special):
            rand[:, col] = s
        return [rand]
    sets = [rand]
    for s in special:
        m = rand.clone()
        m[:, 0] = s
        sets.append(m)
    return sets


@pytest.mark.parametrize("n", [1, 63, 64, 65])
@pytest.mark.parametrize("t", [1, 7, 8, 9, 17])
def test_gae_partial_chunks_and_env_edges(dev, t, n):
    g = torch.Generator().manual_seed(1000 * t + n)
    perm = torch.randperm(n, generator=g)
    for dones in _done_sets(t, n, g):
        r, v, nv = torch.rand(t, n, 1, generator=g), torch.randn(t, n, 1, generator=g), torch.randn(t, n, 1, generator=g)
        ref32 = E.gae(dones.float(), v, r, nv, GAMMA, TAU)
        ref64 = _gae64(dones.double().numpy(), v[..., 0].double().numpy(), r[..., 0].double().numpy(), nv[..., 0].double().numpy())

        def time_major(x):                                  # contiguous (T, N, 1) / (T, N)
            return x.to(dev).contiguous(), None

        def env_major(x):                                   # (N, T + 3) storage with poisoned pad, viewed time-major
            p = Pitched(n, t, t + 3, dev, data=x.reshape(t, n).t(), dtype=x.dtype, poison=NAN if x.dtype.is_floating_point else FLAG)
            vw = p.view.t()
            return (vw.unsqueeze(-1) if x.dim() == 3 else vw), p

        for layout in (time_major, env_major):
            (dd, pd), (vv, pv), (rr, pr), (nn, pn) = layout(dones), layout(v), layout(r), layout(nv)
            for with_ret in (False, True):
                out = ops.discount_values(dd, vv, rr, nn, GAMMA, TAU, return_returns=with_ret)
                adv, ret = out if with_ret else (out, None)
                assert adv.stride() == rr.stride()
                within("gae vs oracle", adv, ref32, ATOL, 1e-5)
                within("gae vs fp64", adv[..., 0], ref64, ATOL, 1e-5)
                if with_ret:
                    within("gae vs oracle", ret, ref32 + v, ATOL, 1e-5)
                    within("gae vs fp64", ret[..., 0], ref64 + v[..., 0].double().numpy(), ATOL, 1e-5)
                # envs are independent: permuting them permutes the outputs bit for bit
                pl = lambda x: layout(x[:, perm])[0]
                out_p = ops.discount_values(pl(dones), pl(v), pl(r), pl(nv), GAMMA, TAU, return_returns=with_ret)
                adv_p, ret_p = out_p if with_ret else (out_p, None)
                assert torch.equal(adv_p.contiguous(), adv[:, perm.to(dev)].contiguous())
                if with_ret:
                    assert torch.equal(ret_p.contiguous(), ret[:, perm.to(dev)].contiguous())
            for p in (pd, pv, pr, pn):                      # inputs: pad columns unread or at least unwritten
                if p is not None:
                    p.assert_poison()
    report("gae vs oracle", "gae vs fp64")


# ================================================================== 2. normaliser
EPS, CLIP = 1e-5, 5.0


def _norm64(x, mean, var, unnorm=False):
    """clamp((x - float(mean)) / sqrt(float(var) + eps), -5, 5), or sqrt(float(var) + eps) * clamp(x, -5, 5) + float(mean): fp64 on fp32-rounded
    statistics, as the module hands them to the formula."""
    m, den = mean.float().double(), torch.sqrt(var.float().double() + EPS)
    x = x.double()
    return den * x.clamp(-CLIP, CLIP) + m if unnorm else ((x - m) / den).clamp(-CLIP, CLIP)


def _owned(rows, nblk):
    per = (rows + nblk - 1) // nblk
    return [(min(rows, b * per), min(rows, (b + 1) * per)) for b in range(nblk)]


def _is_vec4_call(cols, x, x_stride, y, y_stride, y_cols):
    """pulse_rms_normalize's choice of the 16-byte kernel."""
    return (64 <= cols <= 3072 and x_stride % 4 == 0 and y_stride % 4 == 0 and y_cols % 4 == 0 and x.data_ptr() % 16 == 0 and
            y.data_ptr() % 16 == 0 and x_stride >= (cols + 3) // 4 * 4)


def _normalize_case(dev, g, *, rows, cols, x_stride, y_stride, y_cols, nblk, gather, x_lead=0, kernel=None, family):
    src_rows = rows + 5 if gather else rows
    x = torch.randn(src_rows, cols, generator=g) * 3 + 1
    mean = torch.randn(cols, generator=g).double()
    var = (torch.rand(cols, generator=g) + 0.5).double()
    px = Pitched(src_rows, cols, x_stride, dev, data=x, lead=x_lead)
    py = Pitched(rows, y_cols, y_stride, dev)
    idx = torch.randperm(src_rows, generator=g)[:rows] if gather else None
    part_buf, part = flat(nblk * 2 * cols, dev, dtype=torch.float64)
    if kernel == "wide":
        assert cols >= 64 and not _is_vec4_call(cols, px.full, x_stride, py.full, y_stride, y_cols)
    elif kernel == "narrow":
        assert cols < 64
    K.rms_normalize(px.full, mean.to(dev), var.to(dev), rows=rows, cols=cols, x_stride=x_stride, y=py.full, y_stride=y_stride, y_cols=y_cols,
                    row_idx=None if idx is None else idx.to(dev), moment_partials=part.view(nblk, 2, cols), num_blocks=nblk)
    xg = x if idx is None else x[idx]
    within(family + " output", py.view[:, :cols], _norm64(xg, mean, var), 2e-6, 1e-6)
    assert torch.equal(py.view[:, cols:].cpu(), torch.zeros(rows, y_cols - cols))          # the pad is exactly zero
    py.assert_poison()
    px.assert_poison()
    p = part.view(nblk, 2, cols).cpu()
    xd = xg.double()
    for b, (r0, r1) in enumerate(_owned(rows, nblk)):
        if r0 == r1:
            assert torch.equal(p[b], torch.zeros(2, cols, dtype=torch.float64))            # a workgroup without rows leaves exact zeros
    within(family + " moments", p.sum(0)[0], xd.sum(0), 1e-9, 1e-12)
    within(family + " moments", p.sum(0)[1], (xd ** 2).sum(0), 1e-9, 1e-12)
    assert tail_intact(part_buf, nblk * 2 * cols)


WIDE_CASES = [(934, 934, 934, 934, 0), (64, 64, 66, 66, 0), (358, 360, 360, 360, 1),       # (cols, x_stride, y_stride, y_cols, floats in front of x)
              (3072, 3072, 3075, 3072, 0), (3069, 3069, 3072, 3072, 0)]                   # all twelve column slots, without and with a pad


@pytest.mark.parametrize("cols,x_stride,y_stride,y_cols,x_lead", WIDE_CASES)
def test_rms_wide_kernel(dev, cols, x_stride, y_stride, y_cols, x_lead):
    g = torch.Generator().manual_seed(cols + y_stride)
    for rows in (1, 37):
        for nblk in (1, 5, rows + 3):
            for gather in (False, True):
                _normalize_case(dev, g, rows=rows, cols=cols, x_stride=x_stride, y_stride=y_stride, y_cols=y_cols, nblk=nblk, gather=gather,
                                x_lead=x_lead, kernel="wide", family="rms wide")
    report("rms wide output", "rms wide moments")


def test_rms_wide_refuses_the_3075_column_pad(dev):
    """(cols, x_stride, y_stride, y_cols) = (3072, 3072, 3075, 3075): the pad [3072, 3075) lies past the kernels' 3072 column owners and was never
    written; the launch is refused now (pulse_hip.h), so this shape is held to the refusal and the twelve-slot rows above to the numbers."""
    px, py = Pitched(2, 3072, 3072, dev, data=torch.zeros(2, 3072)), Pitched(2, 3075, 3075, dev)
    stat = torch.ones(3072, dtype=torch.float64, device=dev)
    with pytest.raises(PulseLibraryError, match="y_cols 3075 > 3072"):
        K.rms_normalize(px.full, stat, stat, rows=2, cols=3072, x_stride=3072, y=py.full, y_stride=3075, y_cols=3075, num_blocks=1)
    py.assert_poison(0)                                                                    # refused before anything ran


@pytest.mark.parametrize("cols,pitch,kernel", [(934, 960, "vec4"), (1960, 1984, "vec4"), (2320, 2336, "vec4"), (934, 934, "wide")])
def test_rms_unnormalize_wide_rows(dev, cols, pitch, kernel):
    g = torch.Generator().manual_seed(cols + pitch)
    rows, nblk = 37, 3
    for gather in (False, True):
        src_rows = rows + 5 if gather else rows
        z = torch.randn(src_rows, cols, generator=g) * 3
        mean, var = torch.randn(cols, generator=g).double(), (torch.rand(cols, generator=g) + 0.5).double()
        px, py = Pitched(src_rows, cols, pitch, dev, data=z), Pitched(rows, pitch, pitch + (4 if kernel == "vec4" else 3), dev)
        y_stride = py.pitch
        assert _is_vec4_call(cols, px.full, pitch, py.full, y_stride, pitch) == (kernel == "vec4")
        idx = torch.randperm(src_rows, generator=g)[:rows] if gather else None
        K.rms_normalize(px.full, mean.to(dev), var.to(dev), rows=rows, cols=cols, x_stride=pitch, y=py.full, y_stride=y_stride, y_cols=pitch,
                        row_idx=None if idx is None else idx.to(dev), unnorm=True, num_blocks=nblk)
        zg = z if idx is None else z[idx]
        assert (zg.abs() > CLIP).any()                                                     # the clamp is in play
        within(f"rms unnorm {kernel}", py.view[:, :cols], _norm64(zg, mean, var, unnorm=True), 1e-5, 1e-6)
        assert torch.equal(py.view[:, cols:].cpu(), torch.zeros(rows, pitch - cols))
        py.assert_poison()
        px.assert_poison()
    report(f"rms unnorm {kernel}")


@pytest.mark.parametrize("cols", [2, 37, 63])
def test_rms_narrow_kernel(dev, cols):
    g = torch.Generator().manual_seed(cols)
    for rows in (1, 255, 256, 257, 600):
        for nblk in (1, 2, 7):
            _normalize_case(dev, g, rows=rows, cols=cols, x_stride=cols + 1, y_stride=cols + 5, y_cols=cols + 3, nblk=nblk, gather=True,
                            kernel="narrow", family="rms narrow")
    report("rms narrow output", "rms narrow moments")


@pytest.mark.parametrize("count_old", [1.0, 1e6])
@pytest.mark.parametrize("cols", [1, 15, 16, 17, 934])
def test_rms_update_alone(dev, cols, count_old):
    """pulse_rms_update from partials built on the host: the merge of the running statistics with the batch moments
    (_update_mean_var_count_from_moments, running_mean_std.py:56-67 / :98-107) in fp64."""
    batch = 200
    for nblk in (1, 63, 64, 65, 130):
        rs = np.random.RandomState(cols * 1000 + nblk)
        std = rs.uniform(0.5, 2.0, cols)
        mu = rs.choice([-1.0, 1.0], cols) * rs.uniform(0.5, 2.0, cols) * std
        x = rs.standard_normal((batch, cols)) * std + mu
        bm, bv = x.mean(0), x.var(0, ddof=1)
        # |column mean| <= 3 column std: the one-pass variance (s2 - n mean^2) / (n - 1) of the kernel loses at most a factor 1 + mean^2 / var = 10
        assert (np.abs(bm) <= 3.0 * np.sqrt(bv)).all()
        used = rs.permutation(nblk)[: max(1, nblk // 2)]                                  # the other blocks stay empty
        owner = used[rs.randint(0, len(used), batch)]
        part = np.zeros((nblk, 2, cols))
        for b in used:
            part[b, 0], part[b, 1] = x[owner == b].sum(0), (x[owner == b] ** 2).sum(0)
        assert nblk == 1 or (part[:, 0] == 0).all(1).any()
        m_old, v_old = mu * rs.uniform(0.5, 1.5, cols), rs.uniform(0.5, 2.0, cols)
        # the merge in fp64
        delta, tot = bm - m_old, count_old + batch
        want_mean = m_old + delta * batch / tot
        want_var = (v_old * count_old + bv * batch + delta ** 2 * count_old * batch / tot) / tot
        mean_buf, mean = flat(cols, dev, torch.from_numpy(m_old), dtype=torch.float64)
        var_buf, var = flat(cols, dev, torch.from_numpy(v_old), dtype=torch.float64)
        cnt_buf, cnt = flat(1, dev, torch.tensor([count_old], dtype=torch.float64), dtype=torch.float64)
        part_buf, pt = flat(part.size, dev, torch.from_numpy(part.reshape(-1)), dtype=torch.float64)
        K.rms_update(mean, var, cnt, pt.view(nblk, 2, cols), cols, count_old, batch)
        within("rms_update mean", mean, want_mean, rtol=1e-10)
        within("rms_update var", var, want_var, rtol=1e-10)
        assert cnt.item() == count_old + batch                                             # exact
        assert tail_intact(mean_buf, cols) and tail_intact(var_buf, cols) and tail_intact(cnt_buf, 1) and tail_intact(part_buf, part.size)
        assert torch.equal(pt.cpu(), torch.from_numpy(part.reshape(-1)))                   # the partials are read only
    report("rms_update mean", "rms_update var")


# ================================================================== 3. policy head sampler
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


@pytest.mark.parametrize("rows,a", [(1, 1), (15, 15), (16, 16), (17, 17), (33, 69), (5, 153)])
@pytest.mark.parametrize("outputs", ["full", "mus_out", "raw_values", "no_values"])
def test_policy_sample_lane_loop_and_optional_outputs(dev, rows, a, outputs):
    g = torch.Generator().manual_seed(100 * rows + a)
    mu, noise = torch.randn(rows, a, generator=g), torch.randn(rows, a, generator=g)
    logstd = torch.randn(a, generator=g) * 0.3 - 2.0
    vraw = torch.randn(rows, generator=g) * 4                                              # some beyond the +-5 clamp at the larger row counts
    vm, vv = torch.tensor([0.7], dtype=torch.float64), torch.tensor([3.0], dtype=torch.float64)
    pitch = a + 3
    pmu, pnoise = Pitched(rows, a, pitch, dev, data=mu), Pitched(rows, a, a + 1, dev, data=noise)
    pact, psig, pmus = Pitched(rows, a, pitch, dev), Pitched(rows, a, pitch + 1, dev), Pitched(rows, a, pitch + 2, dev)
    pnlp, pval = Pitched(rows, 1, 3, dev), Pitched(rows, 1, 2, dev)
    pvraw = Pitched(rows, 1, 4, dev, data=vraw[:, None])
    ls_buf, ls = flat(a, dev, logstd)
    kw = {}
    if outputs in ("full", "raw_values"):
        kw.update(sigmas=psig.full, sigmas_stride=psig.pitch)
    if outputs == "mus_out":
        kw.update(mus_out=pmus.full, mus_out_stride=pmus.pitch)
    if outputs != "no_values":
        kw.update(value_raw=pvraw.full, value_stride=4, values=pval.full, values_stride=2)
    if outputs in ("full", "mus_out"):
        kw.update(value_mean=vm.to(dev), value_var=vv.to(dev))
    K.policy_sample(pmu.full, pitch, ls, pnoise.full, a + 1, rows, a, pact.full, pitch, pnlp.full, 3, **kw)
    # fp64 model; neglogp is that of the action as stored (fp32)
    m64, sg64 = mu.double(), torch.exp(logstd.double())
    act64 = m64 + sg64 * noise.double()
    z = (act64.float().double() - m64) / sg64
    nlp64 = 0.5 * (z * z).sum(-1) + HALF_LOG_2PI * a + logstd.double().sum()
    within("policy_sample actions", pact.view, act64, 1e-6, 1e-7)
    within("policy_sample neglogp", pnlp.view[:, 0], nlp64, 1e-4, 2e-6)
    pact.assert_poison()
    pnlp.assert_poison()
    if "sigmas" in kw:
        within("policy_sample sigmas", psig.view, sg64.expand(rows, a), rtol=1e-6)
        psig.assert_poison()
    else:
        psig.assert_poison(0)
    if "mus_out" in kw:
        assert torch.equal(pmus.view.cpu(), mu)                                            # a copy
        pmus.assert_poison()
    else:
        pmus.assert_poison(0)
    if outputs in ("full", "mus_out"):
        want = torch.sqrt(vv.float().double() + 1e-5) * vraw.double().clamp(-5, 5) + vm.float().double()
        within("policy_sample values", pval.view[:, 0], want, 2e-6, 1e-7)
        pval.assert_poison()
    elif outputs == "raw_values":
        assert torch.equal(pval.view[:, 0].cpu(), vraw)                                    # no normaliser: the raw value, bit for bit
        pval.assert_poison()
    else:
        pval.assert_poison(0)
    for p in (pmu, pnoise, pvraw):
        p.assert_poison()
    assert tail_intact(ls_buf, a)
    report("policy_sample actions", "policy_sample neglogp", "policy_sample sigmas", "policy_sample values")


# ================================================================== 4. advantage normaliser
@pytest.mark.parametrize("count", [2, 3, 255, 256, 257, 262144, 262147])
def test_advantage_normalize_counts_and_partial_blocks(dev, count):
    g = torch.Generator().manual_seed(count)
    val = torch.randn(count, generator=g)
    ret = val + torch.randn(count, generator=g) * 1.5 + 0.3
    a64 = ret.double() - val.double()
    m, std = a64.mean(), a64.std(unbiased=True)
    assert std.item() >= 0.1
    want = (a64 - m) / (std + 1e-8)
    for nblk in (1, 8, 300):
        ret_buf, r = flat(count, dev, ret)
        val_buf, v = flat(count, dev, val)
        adv_buf, adv = flat(count, dev)
        part_buf, part = flat(2 * nblk, dev, dtype=torch.float64)
        K.advantage_normalize(r, v, adv, part.view(nblk, 2))
        within("advantage_normalize", adv, want, 1e-5, 1e-5)
        assert tail_intact(ret_buf, count) and tail_intact(val_buf, count) and tail_intact(adv_buf, count) and tail_intact(part_buf, 2 * nblk)
    report("advantage_normalize")


# ================================================================== 5. gradient norm + Adam
BIG = 524288 + 259                     # past the 2048-block cap of adam_kernel: the strided second pass


@pytest.mark.parametrize("count", [1, 3, 4, 5, 255, 257, BIG])
def test_sqnorm_and_adam_vs_torch(dev, count):
    for wd in (0.0, 1e-3):
        for max_norm in (0.0, 0.5):
            g = torch.Generator().manual_seed(count + 7)
            p0 = torch.randn(count, generator=g)
            p_ref = torch.nn.Parameter(p0.clone())
            opt = torch.optim.Adam([p_ref], lr=2e-5, eps=1e-8, weight_decay=wd)
            (p_buf, p), (m_buf, m), (v_buf, v) = flat(count, dev, p0), flat(count, dev, torch.zeros(count)), flat(count, dev, torch.zeros(count))
            part_buf, part = flat(64, dev)
            norm_buf, norm_out = flat(1, dev)
            for step in range(1, 4):
                grad = torch.randn(count, generator=g) * (0.3 * step)
                if wd > 0:
                    # The decayed gradient is g * coef + wd * p.  With free signs a few of 524547 elements cancel to the size of eps = 1e-8, where
                    # step = lr * x / (|x| + eps) turns the last bits of the clip coefficient (two fp32 norms agree to ~1e-6) into a fifth of
                    # a step: an ill-conditioned input, not a property of either implementation.  So g takes the sign of p (nothing cancels), at
                    # a norm of about `step` for every count: the clip is active from one element on and wd * p is a sizeable part of the sum
                    # at the large count.
                    grad = torch.sign(p0) * torch.randn(count, generator=g).abs() * (step / math.sqrt(count))
                p_ref.grad = grad.clone()
                ref_norm = torch.nn.utils.clip_grad_norm_([p_ref], max_norm) if max_norm > 0 else grad.double().norm()
                opt.step()
                g_buf, gd = flat(count, dev, grad)
                K.sqnorm_partial(gd, count, part)
                K.adam_step(p, gd, m, v, count, lr=2e-5, step=step, weight_decay=wd, max_norm=max_norm, sqnorm_partials=part, grad_norm_out=norm_out)
                within("sqnorm grad norm", norm_out, ref_norm.reshape(1), rtol=1e-5)
                within("adam_step params", p, p_ref.detach(), 2e-7, 1e-6)
                assert tail_intact(g_buf, count)
            assert tail_intact(p_buf, count) and tail_intact(m_buf, count) and tail_intact(v_buf, count) and tail_intact(part_buf, 64) and tail_intact(norm_buf, 1)
    report("sqnorm grad norm", "adam_step params")


def test_adam_step_multi_with_an_empty_group(dev):
    """Groups of 5, 0 and 524288 + 259 elements in one launch: bit for bit the separate launches; the empty group is legal."""
    sizes = [5, 0, BIG]
    g = torch.Generator().manual_seed(41)

    def fresh():
        gg = torch.Generator().manual_seed(42)
        return [(flat(n, dev, torch.randn(n, generator=gg)), flat(n, dev, torch.zeros(n)), flat(n, dev, torch.zeros(n))) for n in sizes]
    a, b = fresh(), fresh()
    part_buf, part = flat(3 * 64, dev)
    (na_buf, na), (nb_buf, nb) = flat(1, dev), flat(1, dev)
    for step in range(1, 4):
        grads = [flat(n, dev, torch.randn(n, generator=g) * 0.05)[1] for n in sizes]
        for i, (gr, n) in enumerate(zip(grads, sizes)):
            if n:
                K.sqnorm_partial(gr, n, part[64 * i:64 * (i + 1)])
            else:
                part[64 * i:64 * (i + 1)] = 0.0                                            # an empty buffer adds nothing to the joint norm
        kw = dict(lr=3e-4, step=step, weight_decay=1e-3, max_norm=1.0, sqnorm_partials=part)
        for ((_, p), (_, m), (_, v)), gr, n in zip(a, grads, sizes):
            K.adam_step(p, gr, m, v, n, grad_norm_out=na, **kw)
        K.adam_step_multi([(p, gr, m, v, n) for ((_, p), (_, m), (_, v)), gr, n in zip(b, grads, sizes)], grad_norm_out=nb, **kw)
        assert torch.equal(na, nb) and torch.isfinite(na).all()
        for ga, gb, n in zip(a, b, sizes):
            for (buf_a, va), (buf_b, vb) in zip(ga, gb):
                assert torch.equal(va, vb) and torch.isfinite(va).all()
                assert tail_intact(buf_a, n) and tail_intact(buf_b, n)
    assert not torch.equal(a[2][0][1], fresh()[2][0][1])                                   # (the steps moved the parameters)
    assert tail_intact(part_buf, 3 * 64) and tail_intact(na_buf, 1) and tail_intact(nb_buf, 1)


# ================================================================== 6. rollout record
def _rollout_case(dev, n, blocks):
    """Three steps (step 1: nobody done, step 2: everybody done) against the op-by-op reference; ``blocks``: None = the one-workgroup launch that
    updates the meters itself, otherwise the deferred form with that many workgroups and pulse_rollout_meters at the end."""
    g = torch.Generator().manual_seed(10 * n + (blocks or 0))
    t, slot, steps, max_size = 4, 2, 3, 100
    cur_r, cur_l = torch.rand(n, generator=g) * 5, torch.randint(1, 200, (n,), generator=g).float()
    vmean, vvar = torch.tensor([0.3], dtype=torch.float64), torch.tensor([2.5], dtype=torch.float64)
    ref = RolloutReference(cur_r, cur_l, [1.5, 40.0], [120.0, 40.0], max_size, vmean, vvar, 1e-5)
    (cr_buf, cr), (cl_buf, cl) = flat(n, dev, cur_r), flat(n, dev, cur_l)
    meter_r_buf, meter_r = flat(2, dev, torch.tensor([1.5, 40.0]))
    meter_l_buf, meter_l = flat(2, dev, torch.tensor([120.0, 40.0]))
    buf_r, buf_nv = Pitched(n, 1, t, dev, lead=slot, tail=t), Pitched(n, 1, t, dev, lead=slot, tail=t)       # column `slot` of an (n, t) buffer
    buf_d = Pitched(n, 1, t, dev, lead=slot, tail=t, dtype=torch.uint8, poison=FLAG)
    buf_t = Pitched(n, 1, t, dev, lead=slot, tail=t, dtype=torch.uint8, poison=FLAG)
    mask_buf, mask = flat(n, dev, dtype=torch.uint8, poison=FLAG)
    part = torch.full((steps + 1, blocks, 4), NAN, device=dev) if blocks else None
    for step in range(steps):
        rew = torch.rand(n, generator=g)
        dones = (torch.rand(n, generator=g) < 0.3).long()
        if step == 1:
            dones[:] = 0
        if step == 2:
            dones[:] = 1
        term = dones * (torch.rand(n, generator=g) < 0.5).long()
        val = torch.randn(n, 4, generator=g) * 3
        in_bufs = [flat(n, dev, rew), flat(n, dev, dones, dtype=torch.int64, poison=-777), flat(n, dev, term, dtype=torch.int64, poison=-777)]
        pval = Pitched(n, 1, 4, dev, data=val[:, :1])
        K.rollout_record(rewards=in_bufs[0][1], dones=in_bufs[1][1], terminate=in_bufs[2][1], value_raw=pval.full, value_stride=4,
                         value_mean=vmean.to(dev), value_var=vvar.to(dev), value_eps=1e-5, buf_rewards=buf_r.full, buf_next_values=buf_nv.full,
                         buf_dones=buf_d.full, env_stride=t, current_rewards=cr, current_lengths=cl, meter_rewards=meter_r, meter_lengths=meter_l,
                         meter_max_size=max_size, done_mask=mask, buf_terminate=buf_t.full, meter_partials=part[step] if blocks else None)
        nv = ref.step(rew, dones, term, val[:, 0])
        assert torch.equal(buf_r.view[:, 0].cpu(), rew)
        assert torch.equal(buf_d.view[:, 0].cpu(), dones.to(torch.uint8))
        assert torch.equal(buf_t.view[:, 0].cpu(), term.to(torch.uint8))
        within("rollout_record next values", buf_nv.view[:, 0], nv, 1e-6, 1e-6)
        assert torch.equal(cr.cpu(), ref.cur_r) and torch.equal(cl.cpu(), ref.cur_l)
        assert torch.equal(mask.cpu(), dones.to(torch.uint8))
        if blocks:
            assert torch.equal(meter_r.cpu(), torch.tensor([1.5, 40.0])) and torch.equal(meter_l.cpu(), torch.tensor([120.0, 40.0]))   # deferred
            pc = part[step].cpu()
            assert pc[:, 0].sum().item() == float(dones.sum()) and (pc[:, 3] == 0).all()
            per = (n + blocks - 1) // blocks
            idle = torch.tensor([min(n, b * per) >= n for b in range(blocks)])
            assert (pc[idle] == 0).all()                                                   # a workgroup without envs reports nothing
        else:
            within("rollout_record meters", meter_r, ref.meter_r, rtol=2e-5)
            within("rollout_record meters", meter_l, ref.meter_l, rtol=2e-5)
        for (buf, _), poison in zip(in_bufs, (NAN, -777, -777)):
            assert tail_intact(buf, n, poison)
        pval.assert_poison()
    if blocks:
        K.rollout_meters(part[:steps], meter_r, meter_l, max_size)
        within("rollout_record meters", meter_r, ref.meter_r, rtol=2e-5)
        within("rollout_record meters", meter_l, ref.meter_l, rtol=2e-5)
        assert torch.isnan(part[steps]).all()
    for p in (buf_r, buf_nv, buf_d, buf_t):
        p.assert_poison()                                                                  # only column `slot` was written
    assert tail_intact(cr_buf, n) and tail_intact(cl_buf, n) and tail_intact(meter_r_buf, 2) and tail_intact(meter_l_buf, 2)
    assert tail_intact(mask_buf, n, FLAG)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_rollout_record_one_workgroup(dev, n):
    _rollout_case(dev, n, None)
    report("rollout_record next values", "rollout_record meters")


@pytest.mark.parametrize("n,blocks", [(n, 3) for n in (1, 63, 64, 65, 1023, 1024, 1025, 2049)] + [(n, n + 2) for n in (1, 63, 64, 65)])
def test_rollout_record_deferred_meters(dev, n, blocks):
    _rollout_case(dev, n, blocks)
    report("rollout_record next values", "rollout_record meters")


# ================================================================== 7. the two finishing reductions
@pytest.mark.parametrize("count", [1, 2, 3, 5, 7, 69, 1027])
def test_reduce_slabs_scalar_tail(dev, count):
    g = torch.Generator().manual_seed(count)
    stride = (count + 3) // 4 * 4 + 4
    for nslab in (1, 2, 3, 4, 5, 17, 20):
        x = torch.randn(nslab, count, generator=g)
        ps = Pitched(nslab, count, stride, dev, data=x)
        out_buf, out = flat(count, dev)
        K.reduce_slabs(ps.full, nslab, stride, count, out, scale=0.5)
        # every add rounds once: at most nslab roundings of partial sums no larger than sum |x_k|; the scale by 0.5 is exact
        bound = nslab * U24 * x.double().abs().sum(0) * 0.5
        within("reduce_slabs", out, 0.5 * x.double().sum(0), bound=bound.numpy())
        assert tail_intact(out_buf, count)
        ps.assert_poison()
        out2_buf, out2 = flat(count, dev)
        K.reduce_slabs(ps.full, nslab, stride, count, out2, scale=0.5)
        assert torch.equal(out, out2)                                                      # deterministic
    report("reduce_slabs")


@pytest.mark.parametrize("m,n,ld,chunks", [(1, 1, 4, 1), (3, 5, 8, 7), (17, 69, 72, 4), (100, 257, 260, 3)])
def test_colsum_partial_ragged(dev, m, n, ld, chunks):
    g = torch.Generator().manual_seed(m + n)
    x = torch.randn(m, n, generator=g)
    px, pp = Pitched(m, n, ld, dev, data=x), Pitched(chunks, n, n + 3, dev)
    K.colsum_partial(px.full, m, n, ld, chunks, pp.full, n + 3)
    rows = (m + chunks - 1) // chunks
    got = pp.view.cpu()
    for c in range(chunks):
        r0, r1 = min(m, c * rows), min(m, (c + 1) * rows)
        if r0 == r1:
            assert torch.equal(got[c], torch.zeros(n))                                     # an empty chunk writes zeros
        else:
            xc = x[r0:r1].double()
            within("colsum_partial", got[c], xc.sum(0), bound=(m * U24 * xc.abs().sum(0)).numpy())
    within("colsum_partial", got.double().sum(0), x.double().sum(0), bound=(m * U24 * x.double().abs().sum(0)).numpy())
    pp.assert_poison()
    px.assert_poison()
    report("colsum_partial")
