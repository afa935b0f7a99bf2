"""GPU: the discriminator's update pass where its launch plan changes form -- the glue kernels alone against fp64, the weight-gradient and
reduce stage on integer data bit for bit, and the whole pass against the hand-written model of tests/disc_update_model.py.

Every bound is derived from the operation (units of one fp32 rounding, U = 2^-24), from the model's own fp32 run (Y) or from what bf16 rounding
does to the model (E); none from what the kernels gave.  Every check prints its worst error over its bound
(profiles/disc_update_edges.txt records them).  Outputs of the glue kernels sit in NaN-poisoned buffers whose surroundings must survive.
"""
import math
import types

import numpy as np
import pytest
import torch

from pulse_amd import kernels as K
from pulse_amd.learning.amp_agent import AMPAgent
from pulse_amd.learning.disc import DiscNetwork
from tests import disc_update_model as DM

pytestmark = pytest.mark.gpu

NAN = float("nan")
U = 2.0 ** -24                         # one fp32 rounding, relative
TINY = 1e-37                           # fp32 results below the normal range may be flushed to zero
SMALL, SHIPPED = ((64, 32), 70), ((1024, 512), 1960)
COEFS = {"reg": 0.01, "pen": 5.0, "wd": 0.0001, "scale": 5.0}

_WORST = {}


def within(key, got, want, bound):
    """|got - want| <= bound for every element (nothing masked); error where the bound is zero must be zero.  Keeps and prints the worst ratio."""
    f = lambda t: t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)
    got, want = f(got), f(want)
    assert got.shape == want.shape, (key, got.shape, want.shape)
    assert np.isfinite(want).all(), key
    assert np.isfinite(got).all(), f"{key}: non-finite output"
    err = np.abs(got - want)
    lim = np.broadcast_to(f(bound), err.shape)
    exact = lim == 0
    ratio = float((err[~exact] / lim[~exact]).max()) if (~exact).any() else 0.0
    if exact.any() and (err[exact] != 0).any():
        ratio = math.inf
    _WORST[key] = max(_WORST.get(key, 0.0), ratio)
    print(f"[disc_update_edges] {key}: worst error / bound = {ratio:.3e} (max |err| {err.max() if err.size else 0.0:.3e})")
    assert ratio <= 1.0, f"{key}: worst error {ratio:.3f} x its bound (max |err| {err.max():.3e})"


class Pitched:
    """A (rows, cols) matrix with row pitch ``pitch`` inside a flat poisoned buffer: ``lead`` elements in front, ``tail`` behind."""

    def __init__(self, rows, cols, pitch, dev, lead=0, tail=8, dtype=torch.float32, poison=NAN):
        assert pitch >= cols
        self.rows, self.cols, self.pitch, self.lead, self.poison = rows, cols, pitch, lead, poison
        self.flat = torch.full((lead + rows * pitch + tail,), poison, dtype=dtype, device=dev)
        self.full = self.flat[lead: lead + rows * pitch].view(rows, pitch)
        self.view = self.full[:, :cols]

    def assert_poison(self, written=True):
        """Everything outside the view is still poison; the view itself holds no poison (``written``) or nothing but poison."""
        is_p = torch.isnan(self.flat) if isinstance(self.poison, float) else self.flat == self.poison
        inside = torch.zeros(self.flat.shape, dtype=torch.bool, device=self.flat.device)
        inside[self.lead: self.lead + self.rows * self.pitch].view(self.rows, self.pitch)[:, :self.cols] = True
        assert bool(is_p[~inside].all()), "a kernel wrote outside its output"
        assert bool((~is_p[inside]).all() if written else is_p[inside].all()), "an output element was not written" if written else "an output was written"


B16_POISON = 0x7FC0                    # a bf16 NaN


def _bits16(x):
    return x.to(torch.bfloat16).view(torch.int16)


# ================================================================== 3. the glue kernels alone
def _head_logits(b, g):
    """3b logits of scale 3 with the special values spread over the agent and the demo rows (as far as 3b has room)."""
    x = torch.randn(3 * b, generator=g) * 3
    special = torch.tensor([0.0, -0.0, 1e-8, -1e-8, 20.0, -20.0, 90.0, -90.0])
    if b == 1:
        return special[torch.randperm(8, generator=g)[:3]].clone()
    for first, count in ((0, 2 * b), (2 * b, b)):
        k = min(count, 8)
        pos = first + torch.randperm(count, generator=g)[:k]
        x[pos] = special[torch.randperm(8, generator=g)[:k]]
    return x


def _head_model(x, b, scale):
    """fp64 head and the per-element bounds of its fp32 evaluation.  softplus: expf and log1pf within 2 roundings each, the argument's error
    passes through log1p with a factor <= 1, one add: 8 U of the term.  sigmoid: expf (2 U, factor <= 1), add, divide (2 U): 6 U of sg; the
    demo rows' sg - 1 cancels, so its error is 6 U sg + U |sg - 1| absolute; the coefficient scale * 0.5 / n carries 2 roundings, the product 1."""
    x = x.double()
    na = 2 * b
    sp = torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))
    sg = torch.sigmoid(x)
    la, ld = sp[:na].mean(), (sp[na:] - x[na:]).mean()
    stats = torch.stack([0.5 * (la + ld), la, ld, (x[:na] < 0).double().mean(), (x[na:] > 0).double().mean(), x[:na].mean(), x[na:].mean(), torch.zeros((), dtype=torch.float64)])
    e_la = 8 * U * sp[:na].mean() + U * la.abs() + TINY
    e_ld = (8 * U * sp[na:] + U * (sp[na:] - x[na:]).abs()).mean() + U * ld.abs() + TINY           # sp - x: one more rounding of the difference
    sums = 2.0 ** -40                                                                              # the sums themselves are taken in double
    sbound = torch.stack([0.5 * (e_la + e_ld) + U * stats[0].abs(), e_la, e_ld, U * stats[3], U * stats[4], U * stats[5].abs() + sums * x[:na].abs().mean(),
                          U * stats[6].abs() + sums * x[na:].abs().mean(), torch.zeros((), dtype=torch.float64)])
    ga, gd = scale * 0.5 / na, scale * 0.5 / b
    dl = torch.cat([ga * sg[:na], gd * (sg[na:] - 1.0)])
    dbound = torch.cat([ga * 10 * U * sg[:na], gd * (6 * U * sg[na:] + 4 * U * (sg[na:] - 1.0).abs())]) + TINY
    return stats, sbound, dl, dbound


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("b", [1, 341, 342, 683])
def test_disc_head_edges(dev, b, stride):
    g = torch.Generator().manual_seed(100 * b + stride)
    n, scale = 3 * b, 2.5
    x = _head_logits(b, g)
    L = Pitched(n, 1, stride, dev)
    L.view.copy_(x.reshape(-1, 1).to(dev))
    stats64, sbound, dl64, dbound = _head_model(x, b, scale)
    key = f"head b={b} stride={stride}"
    # the fp32 entry
    D = Pitched(n, 1, stride, dev, lead=4)
    S = Pitched(1, 8, 8, dev, lead=4)
    K.disc_head(L.view, b, scale, D.view, S.view.view(-1))
    D.assert_poison(), S.assert_poison()
    within(f"{key} stats", S.view.view(-1), stats64, sbound)
    within(f"{key} dlogits", D.view[:, 0], dl64, dbound)
    d32 = D.view[:, 0].clone()
    # the bf16 entry: with / without the fp32 copy, with / without the bias gradient
    for copy32 in (True, False):
        for with_bias in (True, False):
            D2 = Pitched(n, 1, stride, dev, lead=4)
            D16 = Pitched(n, 1, 32 if stride == 4 else 1, dev, lead=8, dtype=torch.int16, poison=B16_POISON)
            S2, BG = Pitched(1, 8, 8, dev, lead=4), Pitched(1, 1, 1, dev, lead=4)
            K.disc_head_b16(L.view, b, scale, D16.view, S2.view.view(-1), dlogits=D2.view if copy32 else None, bias_grad=BG.view.view(-1) if with_bias else None)
            D2.assert_poison(written=copy32), D16.assert_poison(), S2.assert_poison(), BG.assert_poison(written=with_bias)
            assert torch.equal(S2.view, S.view), "the two entries' statistics differ"
            if copy32:
                assert torch.equal(D2.view[:, 0], d32), "the two entries' fp32 logit gradients differ"
            assert torch.equal(D16.view[:, 0], _bits16(d32)), "bf16 logit gradients: not the RNE of the fp32 ones, bit for bit"
            if with_bias:
                stored = K.from_b16(D16.view[:, 0]).double()
                want = stored.sum()
                within(f"{key} bias_grad", BG.view.view(-1), want.reshape(1), (U * want.abs() + 2.0 ** -40 * stored.abs().sum() + TINY).reshape(1))


PENALTY_SHAPES = [  # (rows, cols, blocks): rows * cols / 4 below, at and above blocks * 256
    (3, 340, 1), (4, 256, 1), (257, 4, 1), (255, 1028, 256), (256, 1024, 256), (257, 1024, 256)]


@pytest.mark.parametrize("rows,cols,blocks", PENALTY_SHAPES)
def test_disc_penalty_edges(dev, rows, cols, blocks):
    g = torch.Generator().manual_seed(rows * 7 + cols)
    scale = 0.37
    Gp = Pitched(rows, cols, cols + 8, dev, lead=4)
    Gp.view.copy_(torch.randn(rows, cols, generator=g).to(dev))
    G64 = Gp.view.double().cpu()
    # the blocks' shares: item i = (row, 4 columns) goes to block (i / 256) mod blocks
    items = (G64 ** 2).reshape(rows * cols // 4, 4).sum(1)
    blk = (torch.arange(items.numel()) // 256) % blocks
    want = torch.zeros(blocks, dtype=torch.float64).index_add_(0, blk, items)
    # all terms positive: a sum of any order errs by at most (its depth) roundings of the total.  Depth: per item 4 squares, 3 adds and the
    # accumulation (5), times the items one thread walks; 6 lane steps, 2 steps across the four waves
    depth = 5 * math.ceil(items.numel() / (blocks * 256)) + 8
    scale32 = torch.tensor(scale, dtype=torch.float32, device=dev)
    dg32 = Gp.view * scale32                                                   # one correctly rounded product: no freedom
    for want32, want16 in ((True, False), (False, True), (True, True), (False, False)):
        P = Pitched(1, blocks, blocks, dev, lead=4)
        O32 = Pitched(rows + 1, cols, cols + 12, dev, lead=4)                  # written from row 1 on: an output offset and a pitch larger than cols
        O16 = Pitched(rows + 2, cols, cols + 20, dev, lead=8, dtype=torch.int16, poison=B16_POISON)
        K.disc_penalty(Gp.view, rows, cols, scale, P.view.view(-1), out32=O32.full if want32 else None, out32_off=O32.pitch, ld32=O32.pitch,
                       out16=O16.full if want16 else None, out16_off=2 * O16.pitch, ld16=O16.pitch)
        P.assert_poison()
        within(f"penalty {rows}x{cols} blocks={blocks} partials", P.view.view(-1), want, depth * U * want + TINY)
        if want32:
            assert torch.equal(O32.view[1:], dg32), "fp32 dg is not the rounded product"
            O32.view[1:] = NAN
        if want16:
            assert torch.equal(O16.view[2:], _bits16(dg32)), "bf16 dg is not the RNE of the rounded product"
            O16.view[2:] = B16_POISON
        assert bool(torch.isnan(O32.flat).all()) and bool((O16.flat == B16_POISON).all()), "written outside the output rows / columns"
    Gp.assert_poison()


REG_CASES = [  # [(offset, length, alpha)], blocks
    ([(0, 1000, 0.5)], 64),
    ([(4, 1024, 0.3), (1101, 999, -2.0)], 1),                               # a 16-byte range and one whose offset and length are not multiples of 4
    ([(0, 4096, 0.0), (4100, 0, 1.5), (4101, 7, 0.7)], 3),                  # alpha 0, a zero-length range
    ([(8, 2000, 0.11), (2010, 3, -0.4), (2016, 1028, 0.9), (3045, 1955, 1e-3)], 5)]


@pytest.mark.parametrize("ranges,blocks", REG_CASES)
@pytest.mark.parametrize("with_grad", [True, False])
def test_disc_reg_edges(dev, ranges, blocks, with_grad):
    g = torch.Generator().manual_seed(len(ranges) * 10 + blocks)
    n = 5000
    flat = torch.full((n,), NAN, device=dev)                                   # NaN outside the ranges: a read past a range shows in its sum
    grad = torch.full((n,), NAN, device=dev)
    for o, ln, _ in ranges:
        flat[o:o + ln] = torch.randn(ln, generator=g).to(dev)
        grad[o:o + ln] = torch.randn(ln, generator=g).to(dev)
    f64, g64 = flat.double().cpu(), grad.double().cpu()
    P = Pitched(blocks, 4, 4, dev, lead=4)
    K.disc_reg(flat, grad if with_grad else None, ranges, P.view)
    P.assert_poison()
    key = f"reg {len(ranges)} ranges blocks={blocks} grad={with_grad}"
    inside = torch.zeros(n, dtype=torch.bool)
    sums = P.view.double().cpu().sum(0)
    for r, (o, ln, al) in enumerate(ranges):
        inside[o:o + ln] = True
        want = (f64[o:o + ln] ** 2).sum()
        depth = 4 * math.ceil(max(ln, 1) / (blocks * 256)) + 8                # per element a square and an add (4 per float4 item), 6 lane steps, 2 wave steps
        within(f"{key} sumsq", sums[r].reshape(1), want.reshape(1), (depth * U * want + (TINY if ln else 0.0)).reshape(1))
        if with_grad:
            al32 = float(np.float32(al))
            upd = g64[o:o + ln] + al32 * f64[o:o + ln]
            # g + alpha w: the product and the sum round once each (or once together when contracted)
            within(f"{key} grad", grad[o:o + ln], upd, U * (al32 * f64[o:o + ln]).abs() + U * upd.abs())
    assert (sums[len(ranges):] == 0).all()
    assert bool(torch.isnan(grad.cpu()[~inside]).all()), "grad written outside the ranges"
    if not with_grad:
        assert torch.equal(grad.cpu()[inside].double(), g64[inside])


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_disc_reward_edges(dev, n, stride):
    g = torch.Generator().manual_seed(n + stride)
    scale, edge = 2.0, math.log(9999.0)                                        # 1 - sigmoid(x) = 1e-4 at x = log(9999): the floor engages above it
    special = torch.tensor([edge - 1e-2, edge - 1e-4, edge, edge + 1e-4, edge + 1e-2, 9.0, 9.5, 90.0, -90.0, 0.0])
    x = torch.randn(n, generator=g) * 6
    k = min(n, special.numel())
    x[torch.randperm(n, generator=g)[:k]] = special[:k] if n > 1 else special[3:4]
    L, O = Pitched(n, 1, stride, dev, lead=4), Pitched(n, 1, stride, dev, lead=4)
    L.view.copy_(x.reshape(-1, 1).to(dev))
    K.disc_reward(L.view, n, scale, O.view)
    O.assert_poison()
    x64 = x.double()
    floor = float(np.float32(0.0001))
    q = torch.clamp(1.0 - torch.sigmoid(x64), min=floor)
    want = -torch.log(q) * scale
    # prob errs by 6 U prob (expf, add, divide), 1 - prob by that plus one rounding: relative to q = max(1 - prob, floor) that is 8 U / q, which
    # the logarithm passes on absolutely; logf and the product add 3 U of the result
    bound = scale * (8 * U / q + 3 * U * torch.log(q).abs()) + TINY
    within(f"reward n={n} stride={stride}", O.view[:, 0], want, bound)
    if n > 1:
        assert (x64 > edge + 5e-3).any() and (x64 < edge - 5e-3).any()


COLSUM_CASES = [  # (m, n, chunks): <4, 8> (64 row lanes) unless ceil(n / 256) * chunks >= 256, then <32, 4> (8 row lanes)
    (33, 70, 7),          # m no multiple of the chunks, 5 rows per chunk (fewer than the row lanes), n no multiple of 8
    (5, 64, 8),           # chunks past the last row: they write zeros
    (1000, 70, 7),
    (2049, 32, 1),        # the one-chunk form of the w3 gradient: the unrolled loop and its tail
    (4101, 2048, 32),     # <32, 4>: 129 rows per chunk
    (4101, 2044, 32),     # <32, 4>, n no multiple of 8
    (70, 2048, 32)]       # <32, 4>, 3 rows per chunk (fewer than the row lanes), chunks 24.. past the last row


@pytest.mark.parametrize("m,n,chunks", COLSUM_CASES)
@pytest.mark.parametrize("w_stride", [0, 1, 32])
def test_colsum_b16_edges(dev, m, n, chunks, w_stride):
    """pulse_colsum_partial_b16 (w_stride 0) and pulse_colsum_weighted_b16 (weights at stride 1 / 32), every chunk's row against fp64."""
    g = torch.Generator().manual_seed(m + n + chunks + w_stride)
    ld = (n + 7) // 8 * 8 + 8
    wide = math.ceil(n / 256) * chunks >= 256
    assert wide == ((n, chunks) in ((2048, 32), (2044, 32)))
    x16 = _bits16(torch.randn(m, ld, generator=g)).to(dev)
    x64 = K.from_b16(x16[:, :n]).double().cpu()
    P = Pitched(chunks, n, n + 5, dev, lead=4)
    if w_stride:
        w16 = torch.full((m, w_stride), B16_POISON, dtype=torch.int16, device=dev)
        w16[:, 0] = _bits16(torch.randn(m, generator=g)).to(dev)
        x64 = x64 * K.from_b16(w16[:, 0]).double().cpu().reshape(-1, 1)                  # bf16 x bf16: exact in fp32
        p = K.Plan()
        p.colsum_weighted_b16(x16, w16, w_stride, m, n, ld, P.flat, chunks, P.pitch, P.lead)
        p.run()
    else:
        K.colsum_partial_b16(x16, m, n, ld, chunks, P.flat, P.pitch, partial_off=P.lead)
    P.assert_poison()
    rows = (m + chunks - 1) // chunks
    lanes, nacc = (8, 4) if wide else (64, 8)
    want, mag = torch.zeros(chunks, n, dtype=torch.float64), torch.zeros(chunks, n, dtype=torch.float64)
    for c in range(chunks):
        seg = x64[c * rows:min(m, (c + 1) * rows)]
        want[c], mag[c] = seg.sum(0), seg.abs().sum(0)
    depth = math.ceil(rows / lanes) + nacc + lanes          # the adds of one lane, its accumulators, the lanes in order: each rounds the running sum once
    within(f"colsum{'_weighted' if w_stride else ''} {m}x{n} chunks={chunks} w_stride={w_stride}", P.view, want, depth * U * mag)


# ================================================================== 4 / 5. DiscNetwork
def _net(dev, shape, weights=None):
    units, amp_dim = shape
    disc = DiscNetwork({"disc": {"units": list(units), "activation": "relu"}}, amp_dim, device=dev)
    if weights is not None:
        disc.load_state_dict(DM.to_state_dict(weights))
    return disc


def device_pass(disc, dev, b, rows, coefs, mixed):
    """One update pass as AMPAgent._extra_gradients runs it (forward, head, backward with the statistics row).  -> CPU snapshot."""
    disc.mixed_precision = bool(mixed)
    ws = disc.workspace(b)
    assert ws["b16"] == bool(mixed)
    k0, r3 = disc.k0, 3 * b
    X = torch.cat(rows, 0).to(dev)
    ws["X"][:r3, :k0] = _bits16(X) if ws["b16"] else X
    logits = disc.forward(ws)
    row = torch.zeros(20, device=dev)
    sqp = torch.zeros(1024, device=dev)
    if ws["b16"]:
        disc.loss_head_b16(ws, logits, b, coefs["scale"], row[:8])
    else:
        K.disc_head(logits, b, coefs["scale"], ws["dlogits"], row[:8])
    disc.backward(ws, coefs["pen"], coefs["reg"], coefs["wd"], scale=coefs["scale"], stats=row[8:17], sq_partials=sqp)
    val = (lambda t: K.from_b16(t)) if ws["b16"] else (lambda t: t)
    out = {"logits": logits[:, 0], "dlogits": val(ws["dL16"][:r3, 0]) if ws["b16"] else ws["dlogits"][:, 0], "G": ws["G"][:, :k0], "row": row,
           "H1": val(ws["H1"][:r3]), "H2": val(ws["H2"][:r3]), "flat_grad": disc.grad, "sq_partials": sqp, "pen_partials": ws["pen_partials"],
           "dg": val(ws["X"][r3:, :k0])}
    out = {k: v.detach().clone().cpu() for k, v in out.items()}
    out["grads"] = {k: disc.gradients()[DM.REF_NAMES[k]].detach().cpu().reshape(-1) if k.startswith("b") else disc.gradients()[DM.REF_NAMES[k]].detach().cpu()
                    for k in DM.NAMES}
    ns = types.SimpleNamespace(_disc_logit_reg=coefs["reg"], _disc_grad_penalty=coefs["pen"], _disc_weight_decay=coefs["wd"])
    out["reported"] = AMPAgent._disc_info(ns, row.unsqueeze(0), b)[0].cpu()
    out["ws"] = ws
    return out


@pytest.fixture(params=["x3", "mfma32"])
def f32_mode(request, monkeypatch):
    """Both fp32 GEMM paths: the three-way bf16 split on the bf16 MFMA (default) and the fp32 MFMA."""
    monkeypatch.setattr(K, "F32_MODE", request.param)
    return request.param


# ---- 4. weight gradients + reduce on integer data
B16_SMALL_B = [1, 5, 47, 48, 95, 96, 191, 192, 383, 384, 511, 512, 767, 768, 1535, 1536]    # both sides of every threshold of the bf16 plans
B16_SHIPPED_B = [47, 48, 383, 384]
F32_SMALL_B = [1, 5, 341, 342]                                                               # 3b >= 1024: 64 bias column-sum chunks instead of one


def _ints(g, r, c, nonzero=False):
    if not nonzero:
        return torch.randint(-3, 4, (r, c), generator=g).float()
    return torch.randint(1, 4, (r, c), generator=g).float() * (torch.randint(0, 2, (r, c), generator=g).float() * 2 - 1)


def _stage_on_integers(dev, shape, b, mixed):
    """One ordinary pass (so that the plans and the cached reduce exist), then ``wgrad`` + that reduce alone on integer operands in [-3, 3]:
    every product and sum is exact in fp32, so the flat gradient equals the integer matrix products bit for bit.  -> the workspace."""
    units, amp_dim = shape
    (u1, u2), k0 = units, amp_dim
    w, rows, _ = DM.draw_case(b, amp_dim, units, seed=b)
    disc = _net(dev, shape, w)
    ws = device_pass(disc, dev, b, rows, COEFS, mixed)["ws"]
    book, S = disc.book, disc.book.split_k
    assert ws["reduce_all_fused"] == ws["b16"], "bf16 storage registers every partial as a region source (widths in whole 4s); fp32 storage registers none"
    assert len(ws["wgrad"].partial_reduces) == (4 if ws["b16"] else 0)
    b3 = disc.l3.b
    if ws["b16"]:
        # the slab contract of loss_head_b16: only slab 0 of the logit bias' range is ever written
        assert bool((book.slabs[1:, b3.off:b3.off + b3.pitch] == 0).all()) and book.slabs[0, b3.off].item() != 0
    g = torch.Generator().manual_seed(7 * b + u1)
    m, r3 = 4 * b, 3 * b
    stack = lambda c: torch.cat([_ints(g, r3, c), _ints(g, b, c, nonzero=True)], 0)         # the penalty rows: nonzero, drawn on their own
    Z1, X, Z2, H1, dL, H2 = stack(u1), stack(k0), stack(u2), stack(u1), stack(1), stack(u2)
    for t in (Z1, X, Z2, H1):
        t[:, 0] = 3.0               # element [0, 0] of the W1 and W2 gradients is 36 b: bf16 holds it for few b only, so a sum that passes through bf16 shows
    put = (lambda dst, src: dst.copy_(_bits16(src).to(dev))) if ws["b16"] else (lambda dst, src: dst.copy_(src.to(dev)))
    put(ws["Z1"], Z1), put(ws["X"][:, :k0], X), put(ws["Z2"], Z2), put(ws["H1"], H1), put(ws["H2"], H2)
    put((ws["dL16"] if ws["b16"] else ws["dL"])[:, 0], dL[:, 0])
    book.slabs.zero_()
    d = lambda t: t.double()
    want = torch.zeros(disc.n_flat, dtype=torch.float64)
    region = lambda p: want[p.off:p.off + p.rows * p.pitch].view(p.rows, p.pitch)
    region(disc.l1.w)[:, :k0] = d(Z1).t() @ d(X)                  # integers of magnitude <= 9 * 4b < 2^24: exact in fp32 and in fp64, in any order
    region(disc.l2.w)[:, :u1] = d(Z2).t() @ d(H1)
    region(disc.l3.w)[:, :u2] = d(dL).t() @ d(H2)
    if ws["b16"]:
        cs1, cs2 = _ints(g, *ws["colsum1"].shape), _ints(g, *ws["colsum2"].shape)       # what the BCE launches leave behind
        ws["colsum1"].copy_(cs1.to(dev)), ws["colsum2"].copy_(cs2.to(dev))
        book.slabs[0, b3.off] = 7.0                                                     # what the loss head leaves behind
        region(disc.l1.b)[0, :u1], region(disc.l2.b)[0, :u2], region(b3)[0, 0] = d(cs1).sum(0), d(cs2).sum(0), 7.0
    else:
        region(disc.l1.b)[0, :u1], region(disc.l2.b)[0, :u2], region(b3)[0, 0] = d(Z1[:r3]).sum(0), d(Z2[:r3]).sum(0), d(dL[:r3]).sum()
    rg = ws["reduce_all"]
    run = lambda al: (ws["wgrad"].run(skip_partial_reduces=ws["reduce_all_fused"]), rg.run(alphas=al, w2_partials=disc._reg_partials))
    disc.grad.fill_(NAN)
    run([0.0] * 6)
    bad = (disc.grad.double().cpu() != want).nonzero().reshape(-1)
    assert bad.numel() == 0, f"alphas 0: {bad.numel()} of {disc.n_flat} gradient elements differ, first at {bad[0].item()}"
    # integer regulariser coefficients on an integer parameter buffer
    fl = torch.randint(-3, 4, (disc.n_flat,), generator=g).float()
    disc.flat.copy_(fl.to(dev))
    alphas = [2.0, 1.0, -3.0, 2.0, 1.0, -2.0]
    for lin, (aw, ab) in zip((disc.l1, disc.l2, disc.l3), zip(alphas[0::2], alphas[1::2])):
        for p, al in ((lin.w, aw), (lin.b, ab)):
            want[p.off:p.off + p.rows * p.pitch] += al * d(fl[p.off:p.off + p.rows * p.pitch])
    disc.grad.fill_(NAN)
    run(alphas)
    bad = (disc.grad.double().cpu() != want).nonzero().reshape(-1)
    assert bad.numel() == 0, f"integer alphas: {bad.numel()} of {disc.n_flat} gradient elements differ, first at {bad[0].item()}"
    sq = disc._reg_partials.double().sum(0).cpu()
    for r, p in enumerate((disc.l1.w, disc.l1.b, disc.l2.w, disc.l2.b, disc.l3.w, disc.l3.b)):
        assert sq[r].item() == (d(fl[p.off:p.off + p.rows * p.pitch]) ** 2).sum().item(), f"sum of squares of region {r}"     # integers again
    return ws


@pytest.mark.parametrize("b", B16_SMALL_B)
def test_wgrad_stage_integers_bf16_storage(dev, b):
    _stage_on_integers(dev, SMALL, b, mixed=True)


@pytest.mark.parametrize("b", B16_SHIPPED_B)
def test_wgrad_stage_integers_bf16_storage_shipped_widths(dev, b):
    _stage_on_integers(dev, SHIPPED, b, mixed=True)


@pytest.mark.parametrize("b", F32_SMALL_B)
def test_wgrad_stage_integers_fp32_storage(f32_mode, dev, b):
    ws = _stage_on_integers(dev, SMALL, b, mixed=False)
    chunks = 64 if 3 * b >= 1024 else 1                                                    # of the bias column sums and of their reduce
    assert ws["wgrad"].ops[-2][3] == "pulse_colsum_partial" and ws["wgrad"].ops[-2][2][4] == chunks and ws["wgrad"].ops[-1][2][1] == chunks


def test_batch_lists_cover_every_plan_form(dev):
    """The lists above are there to cross every threshold of _plans_b16: asserted from the workspaces, so that a threshold that moves takes
    the test with it."""
    splits, chunks, w1_slabs = set(), set(), set()
    for shape, bs in ((SMALL, B16_SMALL_B), (SHIPPED, B16_SHIPPED_B)):
        disc = _net(dev, shape)
        disc.mixed_precision = True
        seen = {}
        for b in bs:
            ws = disc.workspace(b)
            w2_scratch, w3_scratch = ws["_w_scratch"]
            seen[b] = (w2_scratch.shape[0], w3_scratch.shape[0])
            splits.add(w2_scratch.shape[0]), chunks.add(w3_scratch.shape[0]), w1_slabs.add(ws["w_slabs"][0])
            assert w3_scratch.shape[0] == (32 if 4 * b >= 2048 else 1)
        # consecutive pairs of the list sit on the two sides of a threshold: the plan differs across each pair.  (47 | 48 was the step from an
        # unsplit W2 launch to two splits until the unsplit launch -- whose output leaves rounded to bf16 -- was taken out of the plan: the
        # integer-data test at the shipped widths and b = 47 is what found it.  Both sizes stay in the lists.)
        pairs = [(x, y) for x, y in zip(bs, bs[1:]) if y == x + 1]
        assert pairs and all(seen[x] != seen[y] for x, y in pairs if (x, y) != (47, 48)), seen
        assert seen[47] == seen[48] == (2, 1)
    assert splits == {2, 4, 8, 16, 32, 64}, splits                  # every split count wide() can give; none is 1 (see above)
    assert chunks == {1, 32}, chunks
    # (with u2 <= 2047 the plans' weighted column sum stays on the <4, 8> instantiation: <32, 4> is reached by test_colsum_b16_edges alone)


# ---- 5. the whole pass against the model
_CASE = {}


def _drawn(shape, b):
    if (shape, b) not in _CASE:
        units, amp_dim = shape
        _CASE[(shape, b)] = DM.draw_case(b, amp_dim, units, seed=17 * b + units[0])[:2]
    return _CASE[(shape, b)]


def _mask_check(key, got, weights, rows, storage):
    """The device's masks (its stored H1 / H2 > 0) against the fp64 pre-activations of each layer, taken from what the layer read on the device
    (X; the stored H1): where they disagree the pre-activation is within 1e-5 of zero.  Every element is checked."""
    rnd = DM.bf16_rne if storage == "bf16" else (lambda t: t)
    X = rnd(torch.cat(rows, 0).double())
    pre1 = X @ rnd(weights["W1"].double()).t() + weights["b1"].double()
    pre2 = got["H1"].double() @ rnd(weights["W2"].double()).t() + weights["b2"].double()
    m1, m2 = got["H1"] > 0, got["H2"] > 0
    for name, pre, m in (("layer 1", pre1, m1), ("layer 2", pre2, m2)):
        diff = m != (pre > 0)
        worst = pre[diff].abs().max().item() if diff.any() else 0.0
        print(f"[disc_update_edges] {key} {name}: {int(diff.sum())} of {diff.numel()} ReLU masks differ from fp64, largest |pre-activation| there {worst:.3e}")
        assert worst <= 1e-5, f"{key} {name}: a mask differs where the fp64 pre-activation is {worst:.3e}"
    return m1, m2


def _quantities(res):
    """name -> tensor, for a model result or a device snapshot."""
    q = {"logits": res["logits"], "dlogits": res["dlogits"], "G": res["G"], "dg": res["dg"]}
    for i, name in enumerate(DM.REPORTED):
        q[name] = res["reported"][i].reshape(1)
    q["penalty_sum"] = (res["penalty_sum"] if "penalty_sum" in res else res["row"][8]).reshape(1)
    for k in DM.NAMES:
        q["grad " + k] = res["grads"][k]
    return q


def _dist(a, b):
    return (a.detach().double().reshape(-1) - b.detach().double().reshape(-1)).abs().max().item()


def _whole_pass_fp32(dev, shape, b, mode):
    w, rows = _drawn(shape, b)
    got = device_pass(_net(dev, shape, w), dev, b, rows, COEFS, mixed=False)
    key = f"pass fp32 {mode} widths={shape[0]} b={b}"
    masks = _mask_check(key, got, w, rows, "exact")
    m64 = _quantities(DM.disc_update_model(w, rows, COEFS, masks=masks))
    # Y: how far the model's own fp32 evaluation is from fp64, over the three summation orders a split-K sum is free to take
    Y = {k: 0.0 for k in m64}
    for mm in DM.SUM_ORDERS.values():
        m32 = _quantities(DM.disc_update_model(w, rows, COEFS, masks=masks, dtype=torch.float32, mm=mm))
        for k in m64:
            Y[k] = max(Y[k], _dist(m32[k], m64[k]))
    dq = _quantities(got)
    fails = []
    for k in m64:
        err = _dist(dq[k], m64[k])
        ratio = err / (4 * Y[k]) if Y[k] > 0 else (0.0 if err == 0 else math.inf)
        print(f"[disc_update_edges] {key} {k}: |hip - model64| = {err:.3e}, Y = {Y[k]:.3e}, error / (4 Y) = {ratio:.3e}")
        if not ratio <= 1.0:
            fails.append((k, err, Y[k]))
    assert not fails, f"{key}: beyond 4 Y: {fails}"
    # the norm clip's sums of squares are those of the finished gradient (1024 partial sums of positive terms, each over n / 1024 elements)
    n = got["flat_grad"].numel()
    total = (got["flat_grad"].double() ** 2).sum()
    within(f"{key} sq_partials", got["sq_partials"].double().sum().reshape(1), total.reshape(1), ((math.ceil(n / (1024 * 256)) * 5 + 8) * U * total).reshape(1))


@pytest.mark.parametrize("b", [1, 5, 37, 341, 342])
def test_whole_pass_fp32_storage(f32_mode, dev, b):
    _whole_pass_fp32(dev, SMALL, b, f32_mode)


def test_whole_pass_fp32_storage_shipped_widths(dev):
    _whole_pass_fp32(dev, SHIPPED, 342, K.F32_MODE)


def _whole_pass_bf16(dev, shape, b):
    w, rows = _drawn(shape, b)
    got = device_pass(_net(dev, shape, w), dev, b, rows, COEFS, mixed=True)
    key = f"pass bf16 widths={shape[0]} b={b}"
    masks = _mask_check(key, got, w, rows, "bf16")
    exact = DM.disc_update_model(w, rows, COEFS, masks=masks)
    m16 = DM.disc_update_model(w, rows, COEFS, masks=masks, storage="bf16")
    qe, q16, dq = _quantities(exact), _quantities(m16), _quantities(got)
    E = {k: _dist(q16[k], qe[k]) for k in q16}
    bound, why = dict(E), {}
    # Where E cannot hold on a correct pass, the bound is what the model's own quantities justify (profiles/disc_update_edges.txt):
    # -- a tensor of bf16 values moves by one bf16 step of its element wherever the device's fp32 value and the model's fall on the two sides
    #    of a rounding tie, and E (half a step plus what arrives from upstream) is below one step
    for k in ("logits", "dlogits", "G", "dg"):
        bound[k] = E[k] + 2.0 ** (math.floor(math.log2(q16[k].abs().max().item())) - 7)
        why[k] = "E + one bf16 step of the largest element"
    # -- ||w3||^2 is taken from the fp32 parameters, which no storage rounds: E is zero by construction; u2 positive terms, one rounding each
    assert E["disc_logit_loss"] == 0.0
    bound["disc_logit_loss"] = (shape[0][1] + 1) * U * qe["disc_logit_loss"].item()
    why["disc_logit_loss"] = "(u2 + 1) U ||w3||^2"
    # -- an accuracy is a count: every logit within the logits' own bound of zero may fall on the other side, and the ratio is stored in fp32
    near = (q16["logits"].abs() <= E["logits"])
    for k, sl, n in (("disc_agent_acc", slice(0, 2 * b), 2 * b), ("disc_demo_acc", slice(2 * b, 3 * b), b)):
        bound[k] = E[k] + near[sl].sum().item() / n + U
        why[k] = f"E + {int(near[sl].sum())} logits within E(logits) of zero / {n} + U"
    # -- the loss is a sum of terms whose rounding errors may cancel in E: the prediction loss is 1-Lipschitz in every logit (max norm),
    #    the penalty enters with its coefficient, the rest are fp32 sums of the unrounded parameters
    bound["disc_loss"] = E["logits"] + COEFS["pen"] * E["disc_grad_penalty"] + 8 * U * qe["disc_loss"].abs().item()
    why["disc_loss"] = "E(logits) + pen E(penalty) + 8 U loss"
    fails = []
    for k in q16:
        err = _dist(dq[k], q16[k])
        ratio = err / bound[k] if bound[k] > 0 else (0.0 if err == 0 else math.inf)
        print(f"[disc_update_edges] {key} {k}: |hip - model_bf16| = {err:.3e}, E = {E[k]:.3e}, bound = {bound[k]:.3e} ({why.get(k, 'E')}), error / bound = {ratio:.3e}")
        if not ratio <= 1.0:
            fails.append((k, err, bound[k]))
    assert not fails, f"{key}: beyond the bound: {fails}"
    for k in ("logits", "G"):                                  # fp32 buffers holding bf16 values (the unsplit GEMM's output)
        assert torch.equal(DM.bf16_rne(got[k]), got[k]), k


@pytest.mark.parametrize("b", [5, 48, 96, 192, 384, 512])
def test_whole_pass_bf16_storage(dev, b):
    _whole_pass_bf16(dev, SMALL, b)


def test_whole_pass_bf16_storage_shipped_widths(dev):
    _whole_pass_bf16(dev, SHIPPED, 384)


def test_shared_state_across_workspaces_and_a_weight_change(dev):
    """One DiscNetwork, workspaces of different b and of both storages: they share the gradient slabs, the bf16 weight image and the two W^T
    images.  Every pass equals, bit for bit, the same pass on a network built for it alone."""
    w0, _ = _drawn(SMALL, 48)
    disc = _net(dev, SMALL, w0)
    g = torch.Generator().manual_seed(99)
    sequence = [(48, True), (341, False), (384, True), (48, True), ("adam", None), (384, True)]
    for step, (b, mixed) in enumerate(sequence):
        if b == "adam":
            # the parameters change in place, as an optimiser step changes them
            for name in disc.book.params:
                v = disc.book.get(name)
                v.add_((torch.randn(v.shape, generator=g) * 0.02).to(dev))
            continue
        rows = tuple(torch.randn(b, SMALL[1], generator=g).clamp(-5, 5) for _ in range(3))
        got = device_pass(disc, dev, b, rows, COEFS, mixed)
        fresh = _net(dev, SMALL)
        fresh.load_state_dict(disc.state_dict())
        assert torch.equal(fresh.flat, disc.flat)
        want = device_pass(fresh, dev, b, rows, COEFS, mixed)
        for k in ("logits", "dlogits", "G", "dg", "H1", "H2", "row", "flat_grad", "sq_partials", "pen_partials", "reported"):
            assert torch.equal(got[k], want[k]), f"step {step} (b = {b}, bf16 storage {mixed}): {k} differs from a fresh network's"
        assert not torch.isnan(got["flat_grad"]).any() and got["flat_grad"].abs().max() > 0
