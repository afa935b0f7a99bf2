"""Descriptors the product does not reach, drawn from a fixed seed with a bias towards edges (ragged M / N / K around the tile sizes,
long skinny outputs, batches, split-K with empty k ranges, every epilogue / activation, masks, row sums, padded / minimal / unaligned
pitches, offsets, all three compute types, pulse_gemm_x3p with one and three planes), judged against the fp64 model (oracle/gemm_ref.py).
Pitch padding holds NaN (except the zero k padding pulse_gemm_x3p requires), the bytes around every output hold sentinels that must
survive, and where pulse_hip.h promises "same bits" across gemm options (4: matrix outputs, 5, 6, 9) the outputs must be bit-identical."""
import random

import pytest
import torch

from oracle import gemm_ref as GR
from pulse_amd import _lib
from pulse_amd import kernels as K

pytestmark = pytest.mark.gpu

SENT = 1234.5
GUARD = 64
NAN16 = 0x7FC0


@pytest.fixture(autouse=True)
def options():
    yield
    for k in range(16):
        if k != 7:
            K.gemm_set_option(k, 0)


def r4(x):
    return (x + 3) // 4 * 4


def r8(x):
    return (x + 7) // 8 * 8


def pick_mn(rng, skinny=False):
    if skinny:
        return rng.choice([24576, 25000, 32768]), rng.choice([1, 17, 64, 69, 96])
    pool = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257]
    f = lambda: rng.choice(pool) if rng.random() < 0.7 else rng.randint(2, 3000)
    return f(), f()


KS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 934, 1960]


class Buf:
    """A flat device buffer holding one array at an element offset, surrounded by guard elements."""

    def __init__(self, n, dtype, dev, off, fill):
        self.off = GUARD + off
        self.t = torch.full((self.off + n + GUARD,), fill, dtype=dtype, device=dev)
        self.n = n

    @property
    def flat(self):
        return self.t[self.off:]


def operand_f32(g, dev, layout, rows, K_, ld, batch, stride, off):
    n = (batch - 1) * stride + ((rows - 1) * ld + r4(K_) if layout == GR.RED else (K_ - 1) * ld + r4(rows))
    b = Buf(max(n, 1), torch.float32, dev, off, float("nan"))
    v = GR.operand(b.flat, layout, rows, K_, ld, batch, stride)
    v.copy_(torch.randn(v.shape, generator=g).to(dev) / max(1.0, K_ ** 0.5) * (1 + 3 * torch.rand(v.shape, generator=g).to(dev)))
    return b


def draw_f32(rng, g, dev):
    skinny = rng.random() < 0.04
    M, N = pick_mn(rng, skinny)
    K_ = rng.choice(KS)
    ct = rng.choice([GR.COMPUTE_F32X3, GR.COMPUTE_F32X3, GR.COMPUTE_F32, GR.COMPUTE_BF16])
    lay = rng.choice([(0, 0), (0, 1), (1, 1)])
    batch = 1 if skinny else rng.choice([1, 1, 2, 3])
    split = 1
    if lay == (1, 1) and rng.random() < 0.6:
        split = rng.randint(2, 8)
    epi, act = 0, 0
    if split == 1:
        epi = rng.choice([0, 0, 0, 1, 2, 3])
        act = rng.choice([0, 1, 2, 3]) if epi == 0 else 0
    aligned = rng.random() < 0.8
    pad = lambda x: x + rng.choice([0, 0, 4, 12])
    lda = pad(r4(K_) if lay[0] == 0 else r4(M))
    ldb = pad(r4(K_) if lay[1] == 0 else r4(N))
    ldc = pad(r4(N)) if aligned else N + rng.choice([0, 1, 3])
    sa = (M * lda if lay[0] == 0 else K_ * lda) + 4 * rng.randint(0, 3)
    sb = (N * ldb if lay[1] == 0 else K_ * ldb) + 4 * rng.randint(0, 3)
    sc = M * ldc + (4 * rng.randint(0, 2) if aligned else rng.randint(0, 3))
    ss = batch * sc if split > 1 else 0
    oa, ob = 4 * rng.randint(0, 2), 4 * rng.randint(0, 2)
    oc = 4 * rng.randint(0, 2) if aligned else rng.randint(0, 3)
    A = operand_f32(g, dev, lay[0], M, K_, lda, batch, sa, oa)
    B = operand_f32(g, dev, lay[1], N, K_, ldb, batch, sb, ob)
    cn = (batch - 1) * sc + (split - 1) * ss + (M - 1) * ldc + N
    bufs = {"A": A, "B": B, "C": Buf(cn, torch.float32, dev, oc, SENT)}
    kw = dict(M=M, N=N, K=K_, lda=lda, ldb=ldb, ldc=ldc, a_layout=lay[0], b_layout=lay[1], batch=batch, stride_a=sa, stride_b=sb, stride_c=sc,
              split_k=split, split_stride=ss, epilogue=epi, activation=act, compute_bf16=ct == GR.COMPUTE_BF16,
              f32_mode="x3" if ct == GR.COMPUTE_F32X3 else "mfma32", a_off=A.off, b_off=B.off, c_off=bufs["C"].off)
    if epi == 0 and split == 1 and rng.random() < 0.7:
        nb = (r4(N) + 4) * batch
        bufs["bias"] = Buf(nb, torch.float32, dev, 4 * rng.randint(0, 1), float("nan"))
        bufs["bias"].flat[:nb] = torch.randn(nb, generator=g).to(dev)
        kw.update(bias=bufs["bias"].t, bias_off=bufs["bias"].off, stride_bias=r4(N) + 4 if batch > 1 else 0)
    if act >= 2 and (act == 3 or rng.random() < 0.7):
        ldc2 = ldc
        bufs["C2"] = Buf((batch - 1) * sc + (M - 1) * ldc2 + N, torch.float32, dev, oc, SENT)
        kw.update(C2=bufs["C2"].t, c2_off=bufs["C2"].off, ldc2=ldc2, stride_c2=sc)
    mask = aligned and split == 1 and ((epi == 0 and act == 1) or epi == 1) and rng.random() < 0.6
    if epi in (1, 2, 3) and not (epi == 1 and mask):
        ldaux = ldc if aligned else ldc + rng.choice([0, 1])
        n = (batch - 1) * sc + (M - 1) * ldaux + N
        bufs["aux"] = Buf(n, torch.float32, dev, oc if aligned else 0, float("nan"))
        GR.matrix(bufs["aux"].flat, batch, sc, M, N, ldaux).copy_(torch.randn(batch, 1, M, N, generator=g).to(dev) * 2)
        kw.update(aux=bufs["aux"].t, aux_off=bufs["aux"].off, ldaux=ldaux, stride_aux=sc)
    if mask:
        ld_mask = (N + 3) // 4 + rng.choice([0, 1])
        smask = (M + 63) // 64 * 8 * ld_mask
        bufs["relu_mask"] = Buf(batch * smask, torch.int32, dev, 0, 0x12345678)
        if epi == 1:
            bufs["relu_mask"].flat[:batch * smask] = torch.randint(-2 ** 31, 2 ** 31 - 1, (batch * smask,), generator=g, dtype=torch.int32).to(dev)
        kw.update(relu_mask=bufs["relu_mask"].t, mask_off=bufs["relu_mask"].off, ld_mask=ld_mask, stride_mask=smask)
    if lay == (1, 1) and rng.random() < 0.5:
        sr = M + rng.randint(0, 5)
        rsn = (batch - 1) * sr + (split - 1) * ss + M
        bufs["rowsum"] = Buf(rsn, torch.float32, dev, 0, SENT)
        kw.update(rowsum=bufs["rowsum"].t, rowsum_off=bufs["rowsum"].off, stride_rowsum=sr)
    d, _, _ = K.make_gemm_desc(A.t, B.t, bufs["C"].t, **kw)
    return d, bufs


def run_and_judge(d, kind, bufs, launch):
    """Poison the written rectangles, launch, judge (per-element, bf16, mask, plane and split-K rules; the aggregate ratio is measured only:
    at these shapes the device's fp32 matmul yardstick can be far more accurate than an honest sequential accumulation), check sentinels."""
    regions = GR.f32_regions(d) if kind == "f32" else GR.x3p_regions(d)
    for name, (shape, strides, off) in GR.output_rects(d, kind).items():
        v = GR.view(bufs[name].flat, shape, strides, off)
        v.fill_(NAN16 if v.dtype == torch.int16 else float("nan"))
    before = {k: b.t.clone() for k, b in bufs.items() if regions.get(k, (0, 0, 0, False))[3]}
    launch()
    torch.cuda.synchronize()
    mem, outs = {}, {}
    for k, b in bufs.items():
        if k not in regions:
            continue
        if regions[k][3]:
            outs[k] = b.flat
        elif b.t.dtype == torch.int16:
            mem[k] = GR.bf16_bits_to_f64(b.flat)
        elif b.t.dtype in (torch.int32, torch.uint8):
            mem[k] = b.flat.clone()
        else:
            mem[k] = b.flat.double()
    rep = GR.judge(d, kind, mem, outs, aggregate=False)
    # nothing outside the written rectangles changed
    for k, t0 in before.items():
        keep = torch.ones_like(t0, dtype=torch.bool)
        if k in ("relu_mask", "relu_mask8"):
            keep[bufs[k].off:bufs[k].off + bufs[k].n] = False
        else:
            shape, strides, off = GR.output_rects(d, kind)[k]
            GR.view(keep[bufs[k].off:], shape, strides, off).fill_(False)
        if not torch.equal(bufs[k].t[keep], t0[keep]):
            rep["problems"].append(f"{k}: a sentinel outside the written elements changed")
    return rep


def outputs_of(bufs, d, kind):
    return {k: b.t.clone() for k, b in bufs.items() if (GR.f32_regions(d) if kind == "f32" else GR.x3p_regions(d)).get(k, (0, 0, 0, False))[3]}


def test_fuzzed_f32_descriptors(dev):
    rng = random.Random(20261016)
    g = torch.Generator().manual_seed(5)
    lib = _lib.load()
    fails, worst, agg, n = [], 0.0, 0.0, 0
    for i in range(220):
        d, bufs = draw_f32(rng, g, dev)
        st = K._stream()
        launch = lambda: _lib.check(lib.pulse_gemm_f32(__import__("ctypes").byref(d), st), "pulse_gemm_f32")
        rep = run_and_judge(d, "f32", bufs, launch)
        n += 1
        worst, agg = max(worst, rep["worst"]), max(agg, rep["agg"])
        what = f"#{i} M={d.M} N={d.N} K={d.K} b={d.batch} split={d.split_k} lay=({d.a_layout},{d.b_layout}) epi={d.epilogue} act={d.activation} ct={d.compute_type} ldc={d.ldc}"
        if rep["problems"]:
            fails.append(what + ": " + "; ".join(rep["problems"]))
            continue
        if d.compute_type != GR.COMPUTE_F32X3:
            continue
        base = outputs_of(bufs, d, "f32")
        for key, val in ((4, 1), (4, 2), (5, 1), (6, 1)):
            K.gemm_set_option(key, val)
            run_and_judge(d, "f32", bufs, launch)
            K.gemm_set_option(key, 0)
            now = outputs_of(bufs, d, "f32")
            for k in base:
                if k == "rowsum" and key == 4:
                    continue                          # the weight-gradient form's row sums agree to rounding across tilings
                if not torch.equal(torch.nan_to_num(base[k], nan=7.0), torch.nan_to_num(now[k], nan=7.0)):
                    fails.append(what + f": option {key} = {val} changed the bits of {k}")
    print(f"[fuzz] {n} pulse_gemm_f32 descriptors, worst err/tol {worst:.3g}, worst rms/yardstick {agg * GR.RHO:.3g}")
    assert not fails, "\n".join(fails[:20])


def planes_buf(g, dev, layout, rows, K_, ld, batch, stride, planes, off):
    kp = (K_ + 31) // 32 * 32
    extent = (batch - 1) * stride + ((rows - 1) * ld + kp if layout == GR.RED else (K_ - 1) * ld + r8(rows))
    ps = r8(extent) + 8 * (off // 8 + 1)
    b = Buf(ps * planes if planes == 3 else extent, torch.int16, dev, off, NAN16)
    vals = torch.randn(batch, rows, K_, generator=g, dtype=torch.float64).to(dev) / max(1.0, K_ ** 0.5)
    pl = GR.split3(GR.rne_bf16(vals) if planes == 1 else vals.float().double())[:planes]
    for p, v in enumerate(pl):
        flat = b.flat[p * ps:] if planes == 3 else b.flat
        if layout == GR.RED:
            GR.view(flat, (batch, rows, kp), (stride, ld, 1)).fill_(0)
        bits = v.float().to(torch.bfloat16).view(torch.int16)
        GR.operand(flat, layout, rows, K_, ld, batch, stride).copy_(bits)
    return b, ps


def test_fuzzed_x3p_descriptors(dev):
    rng = random.Random(7)
    g = torch.Generator().manual_seed(6)
    lib = _lib.load()
    fails, worst, agg = [], 0.0, 0.0
    for i in range(90):
        M, N = pick_mn(rng)
        K_ = rng.choice(KS)
        planes = rng.choice([1, 3])
        lay = rng.choice([(0, 0), (0, 1), (1, 1)])
        batch = rng.choice([1, 1, 2])
        split = rng.randint(2, 6) if lay == (1, 1) and rng.random() < 0.5 else 1
        epi = rng.choice([0, 0, 1, 2]) if split == 1 else 0
        act = rng.choice([0, 1, 2]) if epi == 0 and split == 1 else 0
        kp = (K_ + 31) // 32 * 32
        lda = (kp if lay[0] == 0 else r8(M)) + rng.choice([0, 8])
        ldb = (kp if lay[1] == 0 else r8(N)) + rng.choice([0, 8])
        sa = (M * lda if lay[0] == 0 else K_ * lda) + 8 * rng.randint(0, 1)
        sb = (N * ldb if lay[1] == 0 else K_ * ldb) + 8 * rng.randint(0, 1)
        A, pa = planes_buf(g, dev, lay[0], M, K_, lda, batch, sa, planes, 8 * rng.randint(0, 1))
        B, pb = planes_buf(g, dev, lay[1], N, K_, ldb, batch, sb, planes, 8 * rng.randint(0, 1))
        ldc = r4(N) + rng.choice([0, 4])
        sc = M * ldc + 4 * rng.randint(0, 1)
        ss = batch * sc if split > 1 else 0
        bufs = {"A": A, "B": B}
        kw = dict(M=M, N=N, K=K_, planes=planes, a_layout=lay[0], b_layout=lay[1], batch=batch, stride_a=sa, stride_b=sb, lda=lda, ldb=ldb,
                  a_off=A.off, b_off=B.off, split_k=split, split_stride=ss, epilogue=epi, activation=act)
        use_c = split > 1 or rng.random() < 0.7
        if use_c:
            bufs["C"] = Buf((batch - 1) * sc + (split - 1) * ss + (M - 1) * ldc + N, torch.float32, dev, 4 * rng.randint(0, 1), SENT)
            kw.update(C=bufs["C"].t, c_off=bufs["C"].off, ldc=ldc, stride_c=sc)
        if split == 1 and (not use_c or rng.random() < 0.5):
            ldcp = r8(N) + rng.choice([0, 8])
            scp = M * ldcp
            cps = batch * scp + 8
            bufs["Cp"] = Buf(cps * planes if planes == 3 else batch * scp, torch.int16, dev, 8, 0x3333)
            kw.update(ldcp=ldcp, stride_cp=scp)
        if epi == 0 and split == 1 and rng.random() < 0.7:
            bufs["bias"] = Buf(batch * N, torch.float32, dev, 0, float("nan"))
            bufs["bias"].flat[:batch * N] = torch.randn(batch * N, generator=g).to(dev)
            kw.update(bias=bufs["bias"].t, bias_off=bufs["bias"].off, stride_bias=N if batch > 1 else 0)
        if act == 2 and use_c:
            bufs["C2"] = Buf((batch - 1) * sc + (M - 1) * ldc + N, torch.float32, dev, bufs["C"].off - GUARD, SENT)
            kw.update(C2=bufs["C2"].t, c2_off=bufs["C2"].off, ldc2=ldc, stride_c2=sc)
        mask = split == 1 and ((epi == 0 and act == 1) or epi == 1) and rng.random() < 0.6
        if epi in (1, 2) and not (epi == 1 and mask):
            b16 = planes == 1 and rng.random() < 0.6
            ldaux = r8(N) if b16 else r4(N)
            n = (batch - 1) * M * ldaux + (M - 1) * ldaux + (r8(N) if b16 else N)
            bufs["aux"] = Buf(n, torch.int16 if b16 else torch.float32, dev, 0, NAN16 if b16 else float("nan"))
            vals = torch.randn(batch, 1, M, N, generator=g).to(dev) * 2
            dst = GR.matrix(bufs["aux"].flat, batch, M * ldaux, M, N, ldaux)
            dst.copy_(vals.to(torch.bfloat16).view(torch.int16) if b16 else vals)
            kw.update(aux=bufs["aux"].t, aux_off=bufs["aux"].off, ldaux=ldaux, stride_aux=M * ldaux)
        if mask:
            ld8 = (N + 7) // 8 + rng.choice([0, 3])
            bufs["relu_mask8"] = Buf(batch * M * ld8, torch.uint8, dev, 0, 0x5A)
            if epi == 1:
                bufs["relu_mask8"].flat[:batch * M * ld8] = torch.randint(0, 256, (batch * M * ld8,), generator=g, dtype=torch.uint8).to(dev)
            kw.update(relu_mask8=bufs["relu_mask8"].t, mask8_off=bufs["relu_mask8"].off, ld_mask8=ld8, stride_mask8=M * ld8)
        if split == 1 and rng.random() < 0.4:
            bufs["out_colsum"] = Buf(batch * GR.x3p_row_tiles(M, N, batch) * N, torch.float32, dev, 0, SENT)
        d = _lib.GemmX3pDesc()
        ptr = lambda name, es: bufs[name].t.data_ptr() + es * bufs[name].off
        d.A, d.B, d.lda, d.ldb, d.a_layout, d.b_layout = ptr("A", 2), ptr("B", 2), lda, ldb, lay[0], lay[1]
        d.a_plane_stride, d.b_plane_stride = (pa, pb) if planes == 3 else (0, 0)
        d.M, d.N, d.K, d.batch, d.planes, d.stride_a, d.stride_b = M, N, K_, batch, planes, sa, sb
        d.split_k, d.split_stride, d.epilogue, d.activation = split, ss, epi, act
        if use_c:
            d.C, d.ldc, d.stride_c = ptr("C", 4), ldc, sc
        if "Cp" in bufs:
            d.Cp, d.ldcp, d.stride_cp = ptr("Cp", 2), kw["ldcp"], kw["stride_cp"]
            d.c_plane_stride = batch * kw["stride_cp"] + 8 if planes == 3 else 0
        if "bias" in bufs:
            d.bias, d.stride_bias = ptr("bias", 4), kw["stride_bias"]
        if "C2" in bufs:
            d.C2, d.ldc2, d.stride_c2 = ptr("C2", 4), ldc, sc
        if "aux" in bufs:
            b16 = bufs["aux"].t.dtype == torch.int16
            d.aux, d.aux_is_bf16, d.ldaux, d.stride_aux = ptr("aux", 2 if b16 else 4), int(b16), kw["ldaux"], kw["stride_aux"]
        if "relu_mask8" in bufs:
            d.relu_mask8, d.ld_mask8, d.stride_mask8 = ptr("relu_mask8", 1), kw["ld_mask8"], kw["stride_mask8"]
        if "out_colsum" in bufs:
            d.out_colsum = ptr("out_colsum", 4)
            d.stride_out_colsum, d.ld_out_colsum = GR.x3p_row_tiles(M, N, batch) * N, N
        st = K._stream()
        launch = lambda: _lib.check(lib.pulse_gemm_x3p(__import__("ctypes").byref(d), st), "pulse_gemm_x3p")
        rep = run_and_judge(d, "x3p", bufs, launch)
        worst, agg = max(worst, rep["worst"]), max(agg, rep["agg"])
        what = f"#{i} M={M} N={N} K={K_} planes={planes} b={batch} split={split} lay={lay} epi={epi} act={act} C={use_c} Cp={'Cp' in bufs}"
        if rep["problems"]:
            fails.append(what + ": " + "; ".join(rep["problems"]))
            continue
        base = outputs_of(bufs, d, "x3p")
        K.gemm_set_option(9, 1)
        run_and_judge(d, "x3p", bufs, launch)
        K.gemm_set_option(9, 0)
        now = outputs_of(bufs, d, "x3p")
        if any(not torch.equal(base[k], now[k]) for k in base):
            fails.append(what + ": option 9 changed the bits")
        for val in (1, 2):
            K.gemm_set_option(3, val)
            r = run_and_judge(d, "x3p", bufs, launch)
            K.gemm_set_option(3, 0)
            if r["problems"]:
                fails.append(what + f" option 3 = {val}: " + "; ".join(r["problems"]))
    print(f"[fuzz] 90 pulse_gemm_x3p descriptors, worst err/tol {worst:.3g}, worst rms/yardstick {agg * GR.RHO:.3g}")
    assert not fails, "\n".join(fails[:20])


def test_fp32_grade_checks_reject_the_bf16_compute_path(dev):
    """The device's own COMPUTE_BF16 output at a cfg2 shape (layer 1 forward: 16384 x 1024 over K = 934) must fail the fp32-grade rules."""
    g = torch.Generator().manual_seed(3)
    M, N, K_ = 16384, 1024, 934
    x = torch.randn(M, 936, generator=g).to(dev)
    w = (torch.randn(N, 936, generator=g) / 30).to(dev)
    c = torch.empty(M, N, device=dev)
    d, _, _ = K.make_gemm_desc(x, w, c, M=M, N=N, K=K_, lda=936, ldb=936, ldc=N, compute_bf16=True)
    d.round_output_bf16 = 0
    K.launch_gemm(d)
    torch.cuda.synchronize()
    d.compute_type = GR.COMPUTE_F32X3                # what the launch would claim if the fp32 path quietly ran on bf16
    rep = GR.judge(d, "f32", {"A": x.reshape(-1).double(), "B": w.reshape(-1).double()}, {"C": c.reshape(-1)})
    assert rep["agg"] > 1 and rep["problems"], rep


def test_b16_silu_gradient_column_sums_are_those_of_the_stored_bf16_output(dev):
    """Regression (found by the fuzz, draw #7 of the x3p stream): with a single-plane Cp output the general epilogue row summed its
    UNROUNDED SiLU-gradient products into out_colsum instead of the bf16 values it stored (pulse_hip.h: "column sums of the OUTPUT as stored")."""
    g = torch.Generator().manual_seed(11)
    M, N, K_ = 256, 128, 40
    a = K.to_b16(torch.randn(M, K_, generator=g).to(dev))
    b = K.to_b16(torch.randn(N, K_, generator=g).to(dev))
    aux = torch.randn(M, N, generator=g).to(dev)
    cp = K.alloc_b16(M, N, dev)
    cs = torch.zeros(K.gemm_x3p_row_tiles(M, N), N, device=dev)
    K.gemm_x3p(a, b, M=M, N=N, K=K_, planes=1, Cp=cp, epilogue=_lib.EPI_SILU_GRAD, aux=aux, ldaux=N, out_colsum=cs)
    torch.cuda.synchronize()
    stored = K.from_b16(cp)[:, :N].double()
    tiles = cs.shape[0]
    h = M // tiles
    want = stored.reshape(tiles, h, N).sum(1)
    lim = GR.gamma(h) * stored.abs().reshape(tiles, h, N).sum(1)
    assert bool(((cs.double() - want).abs() <= lim).all()), float(((cs.double() - want).abs() / lim).max())
