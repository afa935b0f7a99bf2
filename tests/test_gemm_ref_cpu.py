"""The fp64 GEMM model (oracle/gemm_ref.py) against naive index loops on tiny descriptors, and the sensitivity of its checks: every kind
of subtle kernel error the launch audit is meant to catch, faked on the CPU at K = 960 and K = 16384, must be rejected, while an honest
fp32 product passes."""
import math

import numpy as np
import pytest
import torch

from oracle import gemm_ref as GR
from pulse_amd._lib import GemmDesc, GemmX3pDesc


def desc(cls, **kw):
    d = cls()
    d.batch, d.split_k = 1, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def rnd(g, n, scale=1.0):
    return torch.randn(n, generator=g, dtype=torch.float64) * scale


def f32(x):
    return x.float().double()


# ----------------------------------------------------------------------------------------------------------------- naive loops
def silu(z):
    return z / (1 + math.exp(-z))


def dsilu(z):
    s = 1 / (1 + math.exp(-z))
    return s * (1 + z * (1 - s))


def naive(d, A, B, bias=None, aux=None, mask=None, planes=0, kchunk=None, rb16=False):
    """Element loops straight from the pulse_hip.h contracts.  planes: 0 = pulse_gemm_f32 (A / B fp32 values), 1 / 3 = pulse_gemm_x3p."""
    M, N, K, bt, sp = d.M, d.N, d.K, d.batch, d.split_k
    npl = max(planes, 1)

    def a(z, m, k):
        i = z * d.stride_a + (m * d.lda + k if d.a_layout == 0 else k * d.lda + m)
        return sum(float(A[i + p * (d.a_plane_stride if planes == 3 else 0)]) for p in range(npl))

    def b(z, n, k):
        i = z * d.stride_b + (n * d.ldb + k if d.b_layout == 0 else k * d.ldb + n)
        return sum(float(B[i + p * (d.b_plane_stride if planes == 3 else 0)]) for p in range(npl))

    rb = (lambda v: float(GR.rne_bf16(torch.tensor(v)))) if (rb16 or planes == 1) else (lambda v: v)
    C = np.zeros((bt, sp, M, N))
    C2 = np.zeros((bt, 1, M, N))
    bits = np.zeros((bt, M, N), dtype=bool)
    rows = np.zeros((bt, sp, 1, M))
    for z in range(bt):
        for s in range(sp):
            k0, k1 = (s * kchunk, min(K, (s + 1) * kchunk)) if sp > 1 else (0, K)
            k0 = min(k0, K)
            for m in range(M):
                rows[z, s, 0, m] = sum(rb(a(z, m, k)) if rb16 else a(z, m, k) for k in range(k0, k1))
                for n in range(N):
                    acc = sum((rb(a(z, m, k)) * rb(b(z, n, k))) if rb16 else a(z, m, k) * b(z, n, k) for k in range(k0, k1))
                    if sp > 1:
                        C[z, s, m, n] = acc
                        continue
                    if d.epilogue == 0:
                        zz = acc + (float(bias[z * d.stride_bias + n]) if bias is not None else 0.0)
                        if rb16 and d.round_output_bf16 or planes == 1:
                            zz = rb(zz)
                        v = zz
                        if d.activation == 1:
                            v = max(zz, 0.0)
                            bits[z, m, n] = zz > 0
                        elif d.activation == 2:
                            v, C2[z, 0, m, n] = silu(zz), zz
                        elif d.activation == 3:
                            v, C2[z, 0, m, n] = silu(zz), dsilu(zz)
                    else:
                        if rb16 and d.round_output_bf16 or planes == 1:
                            acc = rb(acc)
                        if aux is not None:
                            x = float(aux[z * d.stride_aux + m * d.ldaux + n])
                        if d.epilogue == 1:
                            keep = x > 0 if aux is not None else mask(z, m, n)
                            v = acc if keep else 0.0
                        elif d.epilogue == 2:
                            v = acc * dsilu(x)
                        else:
                            v = acc * x
                    C[z, 0, m, n] = v
    return C, C2, bits, rows


def assert_model(e, ref, exact=False):
    R = e.R.numpy()
    if exact:
        assert np.array_equal(R, ref)
    else:
        np.testing.assert_allclose(R, ref, rtol=1e-12, atol=1e-12)


LAYOUTS = [(0, 0), (0, 1), (1, 1)]


@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("epi,act", [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0)])
@pytest.mark.parametrize("batch", [1, 2])
def test_f32_model_matches_naive_loops(lay, epi, act, batch):
    g = torch.Generator().manual_seed(epi * 31 + act * 7 + batch + 3 * lay[0] + lay[1])
    M, N, K = 5, 6, 9
    lda = 12 if lay[0] == 0 else 8
    ldb = 12 if lay[1] == 0 else 8
    d = desc(GemmDesc, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=7, ldaux=9, a_layout=lay[0], b_layout=lay[1], batch=batch, stride_a=128,
             stride_b=136, stride_c=48, stride_aux=60, stride_bias=8, epilogue=epi, activation=act, compute_type=GR.COMPUTE_F32X3, ldc2=7, stride_c2=48)
    off = 3                                            # element offsets: the pointer names element 3 of the buffer
    A, B, bias, aux = rnd(g, 400), rnd(g, 400), rnd(g, 40), rnd(g, 200)
    mem = {"A": A[off:], "B": B, "C": None}
    if epi == 0:
        mem["bias"] = bias[off:]
    else:
        mem["aux"] = aux[off:]
    if act >= 2:
        mem["C2"] = None
    C, C2, _, _ = naive(d, A[off:], B, bias[off:] if epi == 0 else None, aux[off:] if epi else None)
    out = GR.gemm_f32_model(d, mem)
    assert_model(out["C"], C)
    if act >= 2:
        assert_model(out["C2"], C2)


@pytest.mark.parametrize("compute", [GR.COMPUTE_F32, GR.COMPUTE_BF16, GR.COMPUTE_F32X3])
@pytest.mark.parametrize("K,split", [(40, 1), (40, 3), (17, 8), (100, 2)])
def test_f32_model_split_k_and_rowsum(compute, K, split):
    """Slabs of kchunk = roundup(ceil(K / split), k-tile) rows; split 8 over K = 17 leaves slabs whose k range is empty (zeros)."""
    g = torch.Generator().manual_seed(K * split + compute)
    M, N, batch = 6, 5, 2
    d = desc(GemmDesc, M=M, N=N, K=K, lda=8, ldb=8, ldc=5, a_layout=1, b_layout=1, batch=batch, stride_a=8 * K + 4, stride_b=8 * K, stride_c=400,
             split_k=split, split_stride=30, stride_rowsum=64, compute_type=compute, round_output_bf16=0)
    A, B = rnd(g, 2 * (8 * K + 4)), rnd(g, 2 * 8 * K)
    kc = GR.f32_kchunk(K, split, compute)
    if split == 8:
        assert GR.slab_ranges(K, split, kc)[-1] == (K, K)
    C, _, _, rows = naive(d, A, B, kchunk=kc, rb16=compute == GR.COMPUTE_BF16)
    out = GR.gemm_f32_model(d, {"A": A, "B": B, "C": None, "rowsum": None})
    assert_model(out["C"], C)
    assert_model(out["rowsum"], rows)


@pytest.mark.parametrize("act,epi", [(0, 0), (1, 0), (2, 0), (0, 1)])
def test_f32_bf16_compute_model(act, epi):
    """COMPUTE_BF16: operands RNE-rounded, products exact; round_output_bf16 rounds the product (with its bias) before the epilogue."""
    g = torch.Generator().manual_seed(act + 10 * epi)
    d = desc(GemmDesc, M=4, N=6, K=11, lda=12, ldb=12, ldc=6, ldaux=6, ldc2=6, compute_type=GR.COMPUTE_BF16, round_output_bf16=1, activation=act,
             epilogue=epi)
    A, B, bias, aux = rnd(g, 60), rnd(g, 80), rnd(g, 6), rnd(g, 30)
    mem = {"A": A, "B": B, "C": None}
    mem.update({"bias": bias} if epi == 0 else {"aux": aux})
    C, _, _, _ = naive(d, A, B, bias if epi == 0 else None, aux if epi else None, rb16=True)
    out = GR.gemm_f32_model(d, mem)
    if act in (0, 1):
        # the model's R is exact; the rounded output is within the bf16 rule of it and RNE(R) reproduces the loops' rounding here
        assert GR.bf16_output_problems(torch.tensor(C), out["C"]) == []
    else:
        assert GR.elementwise_ratio(torch.tensor(C), out["C"]) <= 1


def test_f32_mask_layout_round_trip():
    """The bit layout of pulse_gemm_desc.relu_mask: word [((r >> 6) * 8 + (r & 7)) * ld + (c >> 2)], bit 4 ((r >> 3) & 7) + (c & 3)."""
    M, N, ld, batch, stride = 130, 11, 4, 2, 3 * 8 * 4 + 5
    g = torch.Generator().manual_seed(5)
    want = torch.rand(batch, M, N, generator=g) > 0.5
    words = np.zeros(batch * stride + 1, dtype=np.int64)
    for z in range(batch):
        for r in range(M):
            for c in range(N):
                if want[z, r, c]:
                    words[z * stride + ((r >> 6) * 8 + (r & 7)) * ld + (c >> 2)] |= 1 << (4 * ((r >> 3) & 7) + (c & 3))
    got = GR.mask_bits(torch.tensor(words).to(torch.int32), batch, stride, M, N, ld)
    assert torch.equal(got, want)
    d = desc(GemmDesc, M=M, N=N, K=8, lda=8, ldb=8, ldc=N, ld_mask=ld, stride_mask=stride, epilogue=1, batch=batch, stride_a=M * 8,
             stride_b=N * 8, stride_c=M * N, compute_type=GR.COMPUTE_F32X3)
    A, B = rnd(g, batch * M * 8), rnd(g, batch * N * 8)
    C, _, _, _ = naive(d, A, B, mask=lambda z, m, n: bool(want[z, m, n]))
    out = GR.gemm_f32_model(d, {"A": A, "B": B, "C": None, "relu_mask": torch.tensor(words).to(torch.int32)})
    assert_model(out["C"], C)
    assert bool((out["C"].tol[~want[:, None]] == 0).all())          # masked elements must be exact zeros


def test_f32_forward_mask_model():
    g = torch.Generator().manual_seed(9)
    d = desc(GemmDesc, M=70, N=9, K=13, lda=16, ldb=16, ldc=9, activation=1, ld_mask=3, compute_type=GR.COMPUTE_F32X3)
    A, B, bias = rnd(g, 70 * 16), rnd(g, 9 * 16), rnd(g, 9)
    C, _, bits, _ = naive(d, A, B, bias)
    out = GR.gemm_f32_model(d, {"A": A, "B": B, "bias": bias, "C": None, "relu_mask": None})
    assert torch.equal(out["relu_mask"].R > 0, torch.tensor(bits))
    stored = torch.tensor(C[:, 0])
    assert GR.mask_problems(torch.tensor(bits), stored, out["relu_mask"]) == []


def planes_of(x, planes):
    if planes == 1:
        return [GR.rne_bf16(x)]
    return list(GR.split3(f32(x)))


def flat_planes(vals, n, ps):
    """Flat bf16 value buffer: plane p at p * ps."""
    out = torch.zeros(len(vals) * ps if len(vals) > 1 else ps, dtype=torch.float64)
    for p, v in enumerate(vals):
        out[p * ps:p * ps + n] = v[:n]
    return out


@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("epi,act", [(0, 0), (0, 1), (0, 2), (1, 0), (2, 0)])
def test_x3p_model_matches_naive_loops(planes, lay, epi, act):
    g = torch.Generator().manual_seed(planes * 100 + epi * 10 + act + 3 * lay[0] + lay[1])
    M, N, K, batch = 6, 10, 35, 2
    lda = 64 if lay[0] == 0 else 8
    ldb = 64 if lay[1] == 0 else 16
    ea = batch * 520
    eb = batch * 700
    A = flat_planes(planes_of(rnd(g, ea), planes), ea, 1200)
    B = flat_planes(planes_of(rnd(g, eb), planes), eb, 1600)
    d = desc(GemmX3pDesc, M=M, N=N, K=K, lda=lda, ldb=ldb, a_layout=lay[0], b_layout=lay[1], batch=batch, stride_a=520, stride_b=696,
             a_plane_stride=1200, b_plane_stride=1600, ldc=12, stride_c=80, ldc2=12, stride_c2=80, ldaux=16, stride_aux=100, stride_bias=12,
             epilogue=epi, activation=act, planes=planes, ldcp=16, stride_cp=104, c_plane_stride=400, ld_out_colsum=N, stride_out_colsum=N)
    bias, aux = rnd(g, 30), rnd(g, 300)
    mem = {"A": A, "B": B, "C": None, "Cp": None, "out_colsum": None}
    mem.update({"bias": bias} if epi == 0 else {"aux": aux})
    if act == 2:
        mem["C2"] = None
    C, C2, _, _ = naive(d, A, B, bias if epi == 0 else None, aux if epi else None, planes=planes)
    out = GR.gemm_x3p_model(d, mem)
    if planes == 3:
        assert_model(out["C"], C)
        assert_model(out["Cp"], C)
    else:
        assert GR.elementwise_ratio(torch.tensor(C), out["C"]) <= 1
        if out["C"].bf16:
            assert GR.bf16_output_problems(torch.tensor(C), out["C"]) == []
    if act == 2:
        assert GR.elementwise_ratio(torch.tensor(C2), out["C2"]) <= 1
    # out_colsum: one row per row tile (128 rows here), the column sums of the output
    assert out["out_colsum"].R.shape == (batch, 1, GR.x3p_row_tiles(M, N, batch), N)
    np.testing.assert_allclose(out["out_colsum"].R[:, 0, 0].numpy(), out["C"].R[:, 0].sum(1).numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("planes,K,split", [(3, 100, 3), (3, 20, 4), (1, 300, 2), (1, 50, 4)])
def test_x3p_model_split_k(planes, K, split):
    g = torch.Generator().manual_seed(K + split + planes)
    M, N = 7, 9
    d = desc(GemmX3pDesc, M=M, N=N, K=K, lda=8, ldb=16, a_layout=1, b_layout=1, a_plane_stride=K * 8, b_plane_stride=K * 16, planes=planes,
             ldc=12, split_k=split, split_stride=M * 12, stride_c=split * M * 12)
    A = flat_planes(planes_of(rnd(g, K * 8), planes), K * 8, K * 8)
    B = flat_planes(planes_of(rnd(g, K * 16), planes), K * 16, K * 16)
    kc = GR.x3p_kchunk(M, N, K, 1, split, planes)
    C, _, _, _ = naive(d, A, B, kchunk=kc, planes=planes if planes == 3 else 0)
    out = GR.gemm_x3p_model(d, {"A": A, "B": B, "C": None})
    assert_model(out["C"], C)               # slabs stay fp32 (unrounded) in either mode
    if K == 20:
        assert GR.slab_ranges(K, split, kc)[1] == (K, K)


def test_x3p_mask8_layout_and_row_tiles():
    M, N, ld, batch, stride = 9, 19, 4, 2, 40
    g = torch.Generator().manual_seed(2)
    want = torch.rand(batch, M, N, generator=g) > 0.5
    by = np.zeros(batch * stride, dtype=np.int64)
    for z in range(batch):
        for r in range(M):
            for c in range(N):
                if want[z, r, c]:
                    by[z * stride + r * ld + (c >> 3)] |= 1 << (c & 7)
    assert torch.equal(GR.mask8_bits(torch.tensor(by).to(torch.uint8), batch, stride, M, N, ld), want)
    assert GR.x3p_row_tiles(16384, 1024, 1) == 64 and GR.x3p_row_tiles(300, 100, 1) == 3 and GR.x3p_row_tiles(100, 100, 1) == 1


def test_planes_rules():
    g = torch.Generator().manual_seed(4)
    x = f32(rnd(g, 200))
    p = GR.split3(x)
    assert torch.equal(p[0] + p[1] + p[2], x) and GR.planes_problems(*p, value=x) == []
    assert GR.planes_problems(p[0], GR.trunc_bf16(x - p[0]), p[2]) != []


def test_extents_cover_what_the_contract_names():
    d = desc(GemmDesc, A=4096, B=8192, C=16384, M=100, N=50, K=33, lda=36, ldb=36, ldc=52, a_layout=0, b_layout=0, batch=2, stride_a=3600,
             stride_b=1800, stride_c=5200)
    r = GR.f32_regions(d)
    assert r["A"][2] == 3600 + 99 * 36 + 36 and r["B"][2] == 1800 + 49 * 36 + 36 and r["C"][2] == 5200 + 99 * 52 + 50
    d2 = desc(GemmX3pDesc, A=4096, B=8192, C=16384, M=100, N=50, K=33, lda=64, ldb=56, a_layout=0, b_layout=1, a_plane_stride=6400,
              b_plane_stride=33 * 56, planes=3, ldc=52)
    r2 = GR.x3p_regions(d2)
    assert r2["A"][2] == 2 * 6400 + 99 * 64 + 64 and r2["B"][2] == 2 * 33 * 56 + 32 * 56 + 56


# ----------------------------------------------------------------------------------------------------------------- sensitivity
def problem(K, seed, M=48, N=40, bias=False, act=0):
    g = torch.Generator().manual_seed(seed)
    A = f32(rnd(g, M * K))
    B = f32(rnd(g, N * K) / math.sqrt(K))
    d = desc(GemmDesc, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, compute_type=GR.COMPUTE_F32X3, activation=act)
    mem = {"A": A, "B": B, "C": None}
    if bias:
        mem["bias"] = f32(rnd(g, N))
    return d, mem, A.view(M, K), B.view(N, K)


def judge(d, mem, C, extra=None):
    outs = {"C": C.reshape(-1).float()}
    outs.update(extra or {})
    return GR.judge(d, "f32", {k: v for k, v in mem.items() if v is not None}, outs)


def honest(A, B, chunks=4):
    """An honest fp32 product in another association: fp32 partial products of k chunks summed in fp32."""
    K = A.shape[1]
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=torch.float32)
    for c in range(chunks):
        lo, hi = c * K // chunks, (c + 1) * K // chunks
        acc += A[:, lo:hi].float() @ B[:, lo:hi].float().T
    return acc.double()


KS = [960, 16384]


@pytest.mark.parametrize("K", KS)
def test_an_honest_fp32_product_passes(K):
    d, mem, A, B = problem(K, 1, bias=True)
    C = honest(A, B) + mem["bias"]
    rep = judge(d, mem, C)
    assert rep["problems"] == [], rep
    d, mem, A, B = problem(K, 2)
    rep = judge(d, mem, f32(A @ B.T))                 # exact-then-rounded: the best an fp32 output can be
    assert rep["problems"] == [] and rep["agg"] <= 1


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("drop", [(0, 2), (1, 1), (2, 0)])
def test_a_dropped_cross_plane_product_is_rejected(K, drop):
    d, mem, A, B = problem(K, 3)
    pa, pb = GR.split3(A), GR.split3(B)
    C = torch.zeros(A.shape[0], B.shape[0], dtype=torch.float64)
    for i, j in [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]:
        if (i, j) != drop:
            C += pa[i] @ pb[j].T
    rep = judge(d, mem, f32(C))
    assert rep["agg"] > 1 and rep["problems"], rep


@pytest.mark.parametrize("K", KS)
def test_bf16_operands_in_an_fp32_grade_launch_are_rejected(K):
    d, mem, A, B = problem(K, 4)
    rep = judge(d, mem, f32(GR.rne_bf16(A) @ GR.rne_bf16(B).T))
    assert rep["agg"] > 1 and rep["worst"] > 1, rep


@pytest.mark.parametrize("K", KS)
def test_a_missing_k_tile_in_one_slab_is_rejected(K):
    d, mem, A, B = problem(K, 5, M=40, N=32)
    M, N, split = 40, 32, 4
    At, Bt = A.T.contiguous(), B.T.contiguous()            # dW form: both operands [k][out]
    d = desc(GemmDesc, M=M, N=N, K=K, lda=M, ldb=N, ldc=N, a_layout=1, b_layout=1, split_k=split, split_stride=M * N, compute_type=GR.COMPUTE_F32X3)
    mem = {"A": At.reshape(-1), "B": Bt.reshape(-1), "C": None}
    kc = GR.f32_kchunk(K, split, GR.COMPUTE_F32X3)
    slabs = []
    for s, (lo, hi) in enumerate(GR.slab_ranges(K, split, kc)):
        keep = torch.ones(K, dtype=torch.float64)
        keep[:lo] = 0
        keep[hi:] = 0
        if s == 1:
            keep[lo + 16:lo + 32] = 0                       # one 16-deep k tile never accumulated
        slabs.append(f32((A * keep) @ B.T))
    C = torch.stack(slabs)
    rep = judge(d, mem, C)
    assert rep["worst"] > 1 and any("slab sum" in p for p in rep["problems"]), rep
    honest_slabs = torch.stack([f32(A[:, lo:hi] @ B[:, lo:hi].T) for lo, hi in GR.slab_ranges(K, split, kc)])
    assert judge(d, mem, honest_slabs)["problems"] == []


@pytest.mark.parametrize("K", KS)
def test_one_perturbed_element_is_rejected(K):
    d, mem, A, B = problem(K, 6)
    C = f32(A @ B.T)
    S = A.abs() @ B.abs().T
    C[7, 11] += 1e-3 * S[7, 11]
    rep = judge(d, mem, f32(C))
    assert rep["worst"] > 1, rep


@pytest.mark.parametrize("K", KS)
def test_a_bias_shifted_by_one_column_is_rejected(K):
    d, mem, A, B = problem(K, 7, bias=True)
    b = mem["bias"]
    shifted = torch.cat([b[1:], b[:1]])
    rep = judge(d, mem, f32(A @ B.T + shifted))
    assert rep["worst"] > 1, rep


@pytest.mark.parametrize("K", KS)
def test_a_flipped_relu_mask_bit_is_rejected(K):
    d, mem, A, B = problem(K, 8, M=64, N=8, bias=True, act=1)
    d.ld_mask = 2
    z = A @ B.T + mem["bias"]
    C = f32(z.clamp(min=0))
    words = torch.zeros(8 * 2, dtype=torch.int64)
    for r in range(64):
        for c in range(8):
            if z[r, c] > 0:
                words[((r >> 6) * 8 + (r & 7)) * 2 + (c >> 2)] |= 1 << (4 * ((r >> 3) & 7) + (c & 3))
    mem["relu_mask"] = None
    ok = judge(d, mem, C, {"relu_mask": words.clone()})
    assert ok["problems"] == [], ok
    r, c = [int(i) for i in torch.nonzero(z.abs() > 0.5)[3]]      # an element far from zero
    words[((r >> 6) * 8 + (r & 7)) * 2 + (c >> 2)] ^= 1 << (4 * ((r >> 3) & 7) + (c & 3))
    rep = judge(d, mem, C, {"relu_mask": words})
    assert any("relu_mask" in p for p in rep["problems"]), rep


@pytest.mark.parametrize("K", KS)
def test_truncated_bf16_outputs_are_rejected(K):
    d, mem, A, B = problem(K, 9)
    d.compute_type, d.round_output_bf16 = GR.COMPUTE_BF16, 1
    R = GR.rne_bf16(A) @ GR.rne_bf16(B).T
    assert judge(d, mem, GR.rne_bf16(f32(R)))["problems"] == []
    rep = judge(d, mem, GR.trunc_bf16(f32(R)))
    assert any("RNE" in p for p in rep["problems"]), rep
