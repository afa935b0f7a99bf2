"""fp64 model of the two GEMM descriptors (include/pulse_hip.h sections 4 and 4b) and the checks that judge a launch against it.

Device-agnostic torch: every computation runs in float64 on the device of the operand views handed in.  A launch is described by its
descriptor (pulse_amd._lib.GemmDesc / GemmX3pDesc, or anything with the same attribute names) and ``mem``: for every pointer the launch
reads, a FLAT float64 tensor whose element 0 is the element the pointer names (bf16 operands decoded to their values; relu masks as
integer words / bytes).  Optional pointers are "set" exactly when their name is a key of ``mem`` (outputs: any placeholder tensor).

``gemm_f32_model`` / ``gemm_x3p_model`` return {output name: Expect}: the exact value R of every element the launch writes, in the shape
the gather helpers read the device's output in, and the absolute tolerance of each element:

    |C - R| <= tol,   tol = f * gamma(K) * S + C_REL * U * mag,   gamma(K) = U * (GAMMA_A * sqrt(K) + GAMMA_B)

with S = sum_k |A||B| (+ |bias|) in fp64, f the largest derivative of the epilogue's function (SiLU forms) and mag the magnitude the
epilogue's own fp32 arithmetic works at.  Outputs rounded to bf16 add half a bf16 ulp before the epilogue function and are judged by
``bf16_output_problems`` as well.  fp32-grade launches are judged in aggregate too (``aggregate_ratio``) against an honest fp32 product of
the same operands (the same model with ``yardstick=True``: fp32 matmul, TF32 off).  ``judge`` applies every rule to one launch.
"""
import math
from dataclasses import dataclass

import torch

U = 2.0 ** -24                 # unit roundoff of fp32
# Per-element bound.  An fp32 accumulation over K terms drifts like U * sqrt(K) * S in practice; GAMMA_B covers the bias add, the output
# rounding and the MFMA's internal sums at small K.  Measured on every launch of the audited agents (tests/test_gemm_launch_audit_gpu.py)
# at GAMMA_A = 1: the worst honest err / tol was 0.88 (an x3 weight-gradient slab, 512 x 1024 over 2048 of K = 16384), so GAMMA_A = 4
# leaves a 4x margin; the sensitivity cases of tests/test_gemm_ref_cpu.py need tol < 1e-3 * S at K = 16384, i.e. GAMMA_A < ~100.
GAMMA_A, GAMMA_B = 4.0, 8.0
C_REL = 8.0                    # ulps of the epilogue's own fp32 arithmetic (exp, division, products) and the final rounding
# Aggregate rule of fp32-grade launches: rms(C - R) <= RHO * max(rms(Y - R), AGG_FLOOR * U * rms(R)), Y = the fp32 yardstick.  Honest
# kernels measured up to 2.8 x the yardstick's error (x3 weight-gradient slabs of 512 of K against the device's fp32 matmul); one dropped
# cross-plane product is 6.6 - 10 x, bf16-rounded operands > 1000 x (tests/test_gemm_ref_cpu.py, K = 960 and 16384).
RHO = 4.5
AGG_FLOOR = 0.5
# The yardstick itself must be fp32-grade: rms(Y - R) <= KAPPA * U * rms(S).  The device's fp32 matmul measured up to 3.4 U rms(S) on the
# audited launches; a TF32 product is about 2^-11 S / sqrt(K) (>= 64 U S for K <= 16384), a bf16 one 2^-9 S / sqrt(K).
KAPPA = 16.0
BF16_EXACT_FRACTION = 0.98     # bf16-rounded outputs: at least this share equals RNE_bf16(R) exactly (truncation gets ~50 %)
SILU_D1 = 1.1                  # sup |silu'(z)| = 1.0998
SILU_D2 = 0.5                  # sup |silu''(z)| = silu''(0)

RED, OUT = 0, 1
ACT_NONE, ACT_RELU, ACT_SILU, ACT_SILU_D = 0, 1, 2, 3
EPI_BIAS_ACT, EPI_RELU_GRAD, EPI_SILU_GRAD, EPI_MUL_AUX = 0, 1, 2, 3
COMPUTE_F32, COMPUTE_BF16, COMPUTE_F32X3 = 0, 1, 2
BK = {COMPUTE_F32: 32, COMPUTE_BF16: 64, COMPUTE_F32X3: 16}     # k granularity of a pulse_gemm_f32 split-K slab
PK = 32                                                         # k granularity of pulse_gemm_x3p (ring kernel 2 PK, single-plane 3 PK)


def gamma(k):
    return U * (GAMMA_A * math.sqrt(max(int(k), 1)) + GAMMA_B)


# ------------------------------------------------------------------------------------------------------------------- bf16 arithmetic
def rne_bf16(x):
    """Round to bf16, nearest even (values of an fp32 grid)."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def trunc_bf16(x):
    """Round to bf16 towards zero (the error the RNE rule must catch)."""
    b = x.to(torch.float32).view(torch.int32) & -65536
    return b.view(torch.float32).to(torch.float64)


def bf16_half_ulp(x):
    """Half a bf16 ulp at |x| (8 significant bits)."""
    _, e = torch.frexp(x.abs())
    return torch.ldexp(torch.ones_like(x), e - 9) * (x != 0)


def is_bf16(x):
    return rne_bf16(x) == x


def split3(x):
    """The three bf16 planes of fp32 values: x = p0 + p1 + p2 exactly."""
    p0 = rne_bf16(x)
    p1 = rne_bf16(x - p0)
    return p0, p1, rne_bf16(x - p0 - p1)


def bf16_bits_to_f64(t):
    """int16 bf16 bit patterns -> float64 values."""
    return (t.to(torch.int32) << 16).view(torch.float32).to(torch.float64)


# ------------------------------------------------------------------------------------------------------------------- geometry
def view(flat, shape, strides, off=0):
    return flat.as_strided(tuple(int(s) for s in shape), tuple(int(s) for s in strides), flat.storage_offset() + int(off))


def operand(flat, layout, rows, K, ld, batch, stride):
    """(batch, rows, K) view of an operand stored [rows][k] (RED) or [k][rows] (OUT)."""
    if layout == RED:
        return view(flat, (batch, rows, K), (stride, ld, 1))
    return view(flat, (batch, K, rows), (stride, ld, 1)).transpose(1, 2)


def matrix(flat, batch, stride, rows, cols, ld, split=1, split_stride=0, off=0):
    """(batch, split, rows, cols) view of an output stored row-major with pitch ld."""
    return view(flat, (batch, split, rows, cols), (stride, split_stride, ld, 1), off)


def mask_bits(words, batch, stride, M, N, ld):
    """(batch, M, N) bool of a pulse_gemm_desc.relu_mask: word [((r >> 6) * 8 + (r & 7)) * ld + (c >> 2)], bit 4 * ((r >> 3) & 7) + (c & 3)."""
    r = torch.arange(M, device=words.device)[:, None]
    c = torch.arange(N, device=words.device)[None, :]
    widx = ((r >> 6) * 8 + (r & 7)) * ld + (c >> 2)
    bit = 4 * ((r >> 3) & 7) + (c & 3)
    z = torch.arange(batch, device=words.device)[:, None, None] * stride
    w = words.to(torch.int64)[(z + widx[None]).reshape(-1)].reshape(batch, M, N) & 0xffffffff
    return ((w >> bit[None]) & 1) == 1


def mask8_bits(bytes_, batch, stride, M, N, ld):
    """(batch, M, N) bool of a pulse_gemm_x3p_desc.relu_mask8: byte [r * ld + (c >> 3)], bit (c & 7)."""
    r = torch.arange(M, device=bytes_.device)[:, None]
    c = torch.arange(N, device=bytes_.device)[None, :]
    z = torch.arange(batch, device=bytes_.device)[:, None, None] * stride
    b = bytes_.to(torch.int64)[(z + (r * ld + (c >> 3))[None]).reshape(-1)].reshape(batch, M, N) & 0xff
    return ((b >> (c & 7)[None]) & 1) == 1


def f32_kchunk(K, split, compute):
    bk = BK[compute]
    kc = -(-K // split) if split > 0 else K
    kc = -(-kc // bk) * bk
    return kc if kc > 0 else bk


def x3p_big_tiles(M, N, batch, split):
    return ((M + 255) // 256) * ((N + 127) // 128) * batch * split >= 256 or M > 128 * 64


def x3p_row_tiles(M, N, batch):
    """pulse_gemm_x3p_row_tiles: the row count of out_colsum."""
    if M <= 0 or N <= 0 or batch <= 0:
        return 0
    return (M + 255) // 256 if x3p_big_tiles(M, N, batch, 1) else (M + 127) // 128


def x3p_kchunk(M, N, K, batch, split, planes, ring=True):
    single = planes == 1
    kq = 2 * PK if (single and ring and x3p_big_tiles(M, N, batch, split)) else 3 * PK if single else PK
    kc = -(-K // split)
    kc = -(-kc // kq) * kq
    return kc if kc > 0 else kq


def slab_ranges(K, split, kchunk):
    return [(min(K, s * kchunk), min(K, (s + 1) * kchunk)) for s in range(split)]


# ------------------------------------------------------------------------------------------------------------------- the model
@dataclass
class Expect:
    """Exact value and per-element tolerance of one output, shaped like the gather of the device's output."""
    R: torch.Tensor
    tol: torch.Tensor
    bf16: bool = False             # values leave rounded to bf16 (check_bf16_output applies)
    fp32_grade: bool = False       # check_aggregate applies
    K: int = 0                     # reduction length behind the bound
    S: torch.Tensor = None         # sum_k |A||B| (+ |bias|) behind it: the scale of the yardstick rule


def _mm(a, b, yardstick):
    """(batch, M, k) x (batch, N, k) -> (value, S) in fp64; the yardstick is an fp32 product (TF32 off)."""
    if a.shape[-1] == 0:
        z = torch.zeros(a.shape[0], a.shape[1], b.shape[1], dtype=torch.float64, device=a.device)
        return z, z.clone()
    s = torch.matmul(a.abs(), b.abs().transpose(1, 2))
    if yardstick:
        if a.is_cuda:
            assert not torch.backends.cuda.matmul.allow_tf32, "the fp32 yardstick must not run on TF32"
        v = torch.matmul(a.float(), b.float().transpose(1, 2)).double()
    else:
        v = torch.matmul(a, b.transpose(1, 2))
    return v, s


def _fl(x, yardstick):
    return x.float().double() if yardstick else x


def _sig(z):
    return torch.sigmoid(z)


def _epilogue(d, acc, S, K, mem, rounded, yardstick, aux_vals, mask_in):
    """Outputs of one (batch, M, N) accumulator through the descriptor's epilogue (split_k == 1)."""
    g = gamma(K)
    out = {}
    epi, act = int(d.epilogue), int(d.activation)
    if epi == EPI_BIAS_ACT:
        z, tz = acc, g * S
        if rounded:                                   # bf16 autocast: the product leaves rounded, the activation acts on that
            tz = tz + bf16_half_ulp(z.abs() + tz)
            if yardstick:
                z = rne_bf16(z)
        z = _fl(z, yardstick)
        if act == ACT_NONE:
            out["C"] = (z, tz + C_REL * U * z.abs())
        elif act == ACT_RELU:
            r = z.clamp(min=0)
            out["C"] = (r, tz + C_REL * U * r.abs())
            out["_z"] = (z, tz)
        else:
            s = _sig(z)
            r = _fl(z * s, yardstick)
            out["C"] = (r, SILU_D1 * tz + C_REL * U * (z.abs() * s + U))
            if act == ACT_SILU:
                out["C2"] = (z, tz + C_REL * U * z.abs())
            else:
                dv = _fl(s * (1 + z * (1 - s)), yardstick)
                out["C2"] = (dv, SILU_D2 * tz + C_REL * U * (s + z.abs() * s * (1 - s)))
        return out
    if rounded:
        tacc = g * S + bf16_half_ulp(acc.abs() + g * S)
        if yardstick:
            acc = rne_bf16(acc)
    else:
        tacc = g * S
    if epi == EPI_RELU_GRAD:
        keep = (aux_vals > 0) if aux_vals is not None else mask_in
        r = _fl(acc * keep, yardstick)
        out["C"] = (r, (tacc + C_REL * U * acc.abs()) * keep)
    elif epi == EPI_SILU_GRAD:
        s = _sig(aux_vals)
        f = s * (1 + aux_vals * (1 - s))
        r = _fl(acc * f, yardstick)
        out["C"] = (r, tacc * f.abs() + C_REL * U * acc.abs() * (s + aux_vals.abs() * s * (1 - s)))
    else:
        r = _fl(acc * aux_vals, yardstick)
        out["C"] = (r, tacc * aux_vals.abs() + C_REL * U * r.abs())
    return out


def gemm_f32_model(d, mem, yardstick=False):
    """Expected outputs of one pulse_gemm_f32 launch: {"C": (batch, split, M, N), "C2": (batch, 1, M, N), "rowsum": (batch, split, 1, M),
    "relu_mask": (batch, M, N) bool pre-activation sign (with its own tolerance)}."""
    M, N, K, batch, split = int(d.M), int(d.N), int(d.K), int(d.batch), int(d.split_k)
    ct = int(d.compute_type)
    bf = ct == COMPUTE_BF16
    A = operand(mem["A"], int(d.a_layout), M, K, int(d.lda), batch, int(d.stride_a))
    B = operand(mem["B"], int(d.b_layout), N, K, int(d.ldb), batch, int(d.stride_b))
    if bf:                                            # operands are rounded to bf16 on the way in, products exact, fp32 accumulation
        A, B = rne_bf16(A), rne_bf16(B)
    out = {}
    ranges = slab_ranges(K, split, f32_kchunk(K, split, ct))
    if "rowsum" in mem:                               # the bias gradient, summed from the A fragments the kernel holds (bf16-rounded in bf16 mode)
        rs = [_fl(A[..., lo:hi].sum(-1), yardstick) for lo, hi in ranges]
        rt = [gamma(hi - lo) * A[..., lo:hi].abs().sum(-1) + C_REL * U * A[..., lo:hi].sum(-1).abs() for lo, hi in ranges]
        out["rowsum"] = Expect(torch.stack(rs, 1)[:, :, None, :], torch.stack(rt, 1)[:, :, None, :], K=K)
    if split > 1:                                     # slabs: partial sums, no epilogue, never rounded
        vals, tols, ss = [], [], []
        for lo, hi in ranges:
            v, s = _mm(A[..., lo:hi], B[..., lo:hi], yardstick)
            vals.append(_fl(v, yardstick))
            tols.append(gamma(hi - lo) * s + C_REL * U * v.abs())
            ss.append(s)
        out["C"] = Expect(torch.stack(vals, 1), torch.stack(tols, 1), fp32_grade=not bf, K=K, S=torch.stack(ss, 1))
        return out
    acc, S = _mm(A, B, yardstick)
    if "bias" in mem and int(d.epilogue) == EPI_BIAS_ACT:  # the bias is the fp32 initial value of the accumulators
        bias = view(mem["bias"], (batch, 1, N), (int(d.stride_bias), 0, 1))
        acc, S = acc + bias, S + bias.abs()
    aux_vals = view(mem["aux"], (batch, M, N), (int(d.stride_aux), int(d.ldaux), 1)) if "aux" in mem else None
    mask_in = None
    if int(d.epilogue) == EPI_RELU_GRAD and aux_vals is None:
        mask_in = mask_bits(mem["relu_mask"], batch, int(d.stride_mask), M, N, int(d.ld_mask))
    rounded = bf and bool(d.round_output_bf16)
    res = _epilogue(d, acc, S, K, mem, rounded, yardstick, aux_vals, mask_in)
    for k, (r, t) in res.items():
        if k == "_z":
            if "relu_mask" in mem:
                out["relu_mask"] = Expect(r, t, K=K)
        elif k in mem:
            out[k] = Expect(r[:, None], t[:, None], bf16=rounded and k == "C" and _bf16_exact_output(d), fp32_grade=not bf, K=K, S=S[:, None])
    return out


def _bf16_exact_output(d):
    """Outputs that are the rounded product itself (or it times 0 / 1): ReLU / none forward, ReLU gradient."""
    return (int(d.epilogue) == EPI_BIAS_ACT and int(d.activation) in (ACT_NONE, ACT_RELU)) or int(d.epilogue) == EPI_RELU_GRAD


def x3p_operand(flat, layout, rows, K, ld, batch, stride, plane_stride, planes):
    v = operand(flat, layout, rows, K, ld, batch, stride)
    if planes == 1:
        return v
    return v + operand(flat[plane_stride:], layout, rows, K, ld, batch, stride) + operand(flat[2 * plane_stride:], layout, rows, K, ld, batch, stride)


def gemm_x3p_model(d, mem, yardstick=False, ring=True):
    """Expected outputs of one pulse_gemm_x3p launch: {"C": (batch, split, M, N), "C2", "Cp" (the value the planes hold; bf16 for
    planes = 1), "out_colsum": (batch, 1, tiles, N), "relu_mask8": (batch, M, N) pre-activation sign}.  mem["A"] / ["B"] / ["aux"
    with aux_is_bf16]: decoded bf16 values, planes at their plane strides."""
    M, N, K, batch, split = int(d.M), int(d.N), int(d.K), int(d.batch), int(d.split_k)
    planes = 1 if int(d.planes) == 1 else 3
    A = x3p_operand(mem["A"], int(d.a_layout), M, K, int(d.lda), batch, int(d.stride_a), int(d.a_plane_stride), planes)
    B = x3p_operand(mem["B"], int(d.b_layout), N, K, int(d.ldb), batch, int(d.stride_b), int(d.b_plane_stride), planes)
    out = {}
    if split > 1:
        kc = x3p_kchunk(M, N, K, batch, split, planes, ring)
        vals, tols, ss = [], [], []
        for lo, hi in slab_ranges(K, split, kc):
            v, s = _mm(A[..., lo:hi], B[..., lo:hi], yardstick)
            vals.append(_fl(v, yardstick))
            tols.append(gamma(hi - lo) * s + C_REL * U * v.abs())
            ss.append(s)
        out["C"] = Expect(torch.stack(vals, 1), torch.stack(tols, 1), fp32_grade=planes == 3, K=K, S=torch.stack(ss, 1))
        return out
    acc, S = _mm(A, B, yardstick)
    if "bias" in mem and int(d.epilogue) == EPI_BIAS_ACT:
        bias = view(mem["bias"], (batch, 1, N), (int(d.stride_bias), 0, 1))
        acc, S = acc + bias, S + bias.abs()
    aux_vals = view(mem["aux"], (batch, M, N), (int(d.stride_aux), int(d.ldaux), 1)) if "aux" in mem else None
    mask_in = None
    if int(d.epilogue) == EPI_RELU_GRAD and aux_vals is None:
        mask_in = mask8_bits(mem["relu_mask8"], batch, int(d.stride_mask8), M, N, int(d.ld_mask8))
    rounded = planes == 1
    res = _epilogue(d, acc, S, K, mem, rounded, yardstick, aux_vals, mask_in)
    exact16 = rounded and _bf16_exact_output(d)
    for k, (r, t) in res.items():
        if k == "_z":
            if "relu_mask8" in mem:
                out["relu_mask8"] = Expect(r, t, K=K)
        elif k in mem:
            out[k] = Expect(r[:, None], t[:, None], bf16=exact16 and k == "C", fp32_grade=planes == 3, K=K, S=S[:, None])
    r, t = res["C"]
    if "Cp" in mem:
        if planes == 1:                               # one bf16 matrix: the stored output rounded once more (a no-op for exact16 outputs)
            tp = t + bf16_half_ulp(r.abs() + t)
            out["Cp"] = Expect((rne_bf16(r) if yardstick else r)[:, None], tp[:, None], bf16=exact16, K=K)
        else:
            out["Cp"] = Expect(r[:, None], t[:, None], fp32_grade=True, K=K, S=S[:, None])
    if "out_colsum" in mem:
        tiles = x3p_row_tiles(M, N, batch)
        h = 256 if tiles != (M + 127) // 128 else 128
        pad = tiles * h - M
        tr = torch.nn.functional.pad(t, (0, 0, 0, pad)).reshape(batch, tiles, h, N)
        rr = torch.nn.functional.pad(r, (0, 0, 0, pad)).reshape(batch, tiles, h, N)
        if rounded and yardstick:
            rr = rne_bf16(rr)
        cs = _fl(rr.sum(2), yardstick)
        ct = tr.sum(2) + gamma(h) * rr.abs().sum(2) + (bf16_half_ulp(rr.abs() + tr).sum(2) if rounded else 0)
        out["out_colsum"] = Expect(cs[:, None], ct[:, None], K=K)
    return out


# ------------------------------------------------------------------------------------------------------------------- the checks
def rms(x):
    return float(x.double().pow(2).mean().sqrt()) if x.numel() else 0.0


def elementwise_ratio(C, e):
    """Worst |C - R| / tol (<= 1 passes; an element with tol 0 must be exact; a NaN anywhere fails)."""
    err = (C.double() - e.R).abs()
    if torch.isnan(err).any():
        return math.inf
    over = err > e.tol
    if over.any():
        t = e.tol[over]
        return math.inf if bool((t == 0).any()) else float((err[over] / t).max())
    t = e.tol
    nz = t > 0
    return float((err[nz] / t[nz]).max()) if bool(nz.any()) else 0.0


def aggregate_ratio(C, R, Y):
    """rms(C - R) / (RHO * max(rms(Y - R), floor)): <= 1 passes."""
    den = max(rms(Y - R), AGG_FLOOR * U * rms(R))
    num = rms(C.double() - R)
    if den == 0.0:
        return 0.0 if num == 0.0 else math.inf
    return num / (RHO * den)


def yardstick_ratio(Y, R, S):
    """rms(Y - R) / (KAPPA * U * rms(S)): <= 1 means the yardstick is fp32-grade."""
    den = KAPPA * U * rms(S)
    num = rms(Y - R)
    return 0.0 if num == 0.0 else (num / den if den > 0 else math.inf)


def bf16_output_problems(C, e):
    """The bf16-output rule: every value bf16-representable, |C - R| <= half ulp(R) + tol, >= BF16_EXACT_FRACTION equal RNE_bf16(R)."""
    C = C.double()
    bad = []
    if not bool(is_bf16(C).all()):
        bad.append(f"{int((~is_bf16(C)).sum())} values not bf16-representable")
    err = (C - e.R).abs()
    lim = bf16_half_ulp(e.R) + e.tol
    if bool((err > lim).any()) or torch.isnan(err).any():
        bad.append(f"{int((err > lim).sum())} values off by more than half a bf16 ulp + tol")
    n = C.numel()
    if n:
        eq = float((C == rne_bf16(e.R)).double().mean())
        if eq < BF16_EXACT_FRACTION:
            bad.append(f"only {eq:.3f} of the values equal RNE_bf16(R)")
    return bad


def mask_problems(bits, stored, e):
    """A forward mask bit equals (stored C > 0) everywhere; it may disagree with the sign of the fp64 pre-activation only where that is
    within its own bound of zero."""
    bad = []
    pos = stored.double() > 0
    if not torch.equal(bits, pos):
        bad.append(f"{int((bits != pos).sum())} bits differ from the stored output's sign")
    flip = bits != (e.R > 0)
    if bool((flip & (e.R.abs() > e.tol)).any()):
        bad.append(f"{int((flip & (e.R.abs() > e.tol)).sum())} bits disagree with a pre-activation clear of zero")
    return bad


def planes_problems(p0, p1, p2, value=None):
    """Output planes are exact: p0 = RNE(v), p1 = RNE(v - p0), p2 = RNE(v - p0 - p1), v = p0 + p1 + p2 (= the stored fp32 output if given)."""
    v = p0 + p1 + p2
    bad = []
    if value is not None and not torch.equal(v, value.double()):
        bad.append(f"{int((v != value.double()).sum())} plane sums differ from the stored output")
    q0, q1, q2 = split3(v)
    if not (torch.equal(q0, p0) and torch.equal(q1, p1) and torch.equal(q2, p2)):
        bad.append("planes are not the RNE split of their sum")
    return bad


# ------------------------------------------------------------------------------------------------------------------- extents
def _r4(x):
    return (x + 3) // 4 * 4


def _r8(x):
    return (x + 7) // 8 * 8


def f32_regions(d):
    """Every array a pulse_gemm_f32 launch touches: {name: (address, bytes per element, elements from the address, written)}.  Extents as
    the kernels read them: reduction-contiguous rows up to roundup4(K), [k][out] rows up to roundup4(extent)."""
    M, N, K, bt, sp = int(d.M), int(d.N), int(d.K), int(d.batch), int(d.split_k)
    akc, bkc = int(d.a_layout) == RED, int(d.b_layout) == RED
    reg = {}

    def add(name, ptr, es, n, out):
        if ptr:
            reg[name] = (int(ptr), es, int(n), out)
    add("A", d.A, 4, (bt - 1) * d.stride_a + ((M - 1) * d.lda + _r4(K) if akc else (K - 1) * d.lda + _r4(M)) if K else 0, False)
    add("B", d.B, 4, (bt - 1) * d.stride_b + ((N - 1) * d.ldb + _r4(K) if bkc else (K - 1) * d.ldb + _r4(N)) if K else 0, False)
    add("C", d.C, 4, (bt - 1) * d.stride_c + (sp - 1) * d.split_stride + (M - 1) * d.ldc + N, True)
    if int(d.epilogue) == EPI_BIAS_ACT and int(d.activation) >= ACT_SILU:
        add("C2", d.C2, 4, (bt - 1) * d.stride_c2 + (M - 1) * d.ldc2 + N, True)
    if int(d.epilogue) == EPI_BIAS_ACT:
        add("bias", d.bias, 4, (bt - 1) * d.stride_bias + N, False)
    else:
        add("aux", d.aux, 4, (bt - 1) * d.stride_aux + (M - 1) * d.ldaux + N, False)
    add("rowsum", d.rowsum, 4, (bt - 1) * d.stride_rowsum + (sp - 1) * d.split_stride + M, True)
    fwd = int(d.epilogue) == EPI_BIAS_ACT and int(d.activation) == ACT_RELU
    if d.relu_mask and (fwd or (int(d.epilogue) == EPI_RELU_GRAD and not d.aux)):
        add("relu_mask", d.relu_mask, 4, (bt - 1) * d.stride_mask + ((M + 63) // 64 * 8 - 1) * d.ld_mask + (N + 3) // 4, fwd)
    return reg


def x3p_regions(d):
    """The same for pulse_gemm_x3p: bf16 operands with their planes, reduction-contiguous rows up to roundup32(K) (the zero padding is
    read), [k][out] rows up to roundup8(extent); Cp rows up to roundup8(N) (the pad columns are written as zeros)."""
    M, N, K, bt, sp = int(d.M), int(d.N), int(d.K), int(d.batch), int(d.split_k)
    npl = 1 if int(d.planes) == 1 else 3
    akc, bkc = int(d.a_layout) == RED, int(d.b_layout) == RED
    kp = (K + PK - 1) // PK * PK
    reg = {}

    def add(name, ptr, es, n, out):
        if ptr:
            reg[name] = (int(ptr), es, int(n), out)
    pa = (npl - 1) * d.a_plane_stride if npl == 3 else 0
    pb = (npl - 1) * d.b_plane_stride if npl == 3 else 0
    add("A", d.A, 2, pa + (bt - 1) * d.stride_a + ((M - 1) * d.lda + kp if akc else (K - 1) * d.lda + _r8(M)) if K else 0, False)
    add("B", d.B, 2, pb + (bt - 1) * d.stride_b + ((N - 1) * d.ldb + kp if bkc else (K - 1) * d.ldb + _r8(N)) if K else 0, False)
    add("C", d.C, 4, (bt - 1) * d.stride_c + (sp - 1) * d.split_stride + (M - 1) * d.ldc + N, True)
    add("Cp", d.Cp, 2, ((npl - 1) * d.c_plane_stride if npl == 3 else 0) + (bt - 1) * d.stride_cp + (M - 1) * d.ldcp + _r8(N), True)
    if int(d.epilogue) == EPI_BIAS_ACT and int(d.activation) == ACT_SILU:
        add("C2", d.C2, 4, (bt - 1) * d.stride_c2 + (M - 1) * d.ldc2 + N, True)
    if int(d.epilogue) == EPI_BIAS_ACT:
        add("bias", d.bias, 4, (bt - 1) * d.stride_bias + N, False)
    elif d.aux:
        add("aux", d.aux, 2 if d.aux_is_bf16 else 4, (bt - 1) * d.stride_aux + (M - 1) * d.ldaux + (_r8(N) if d.aux_is_bf16 else N), False)
    if d.out_colsum:
        add("out_colsum", d.out_colsum, 4, (bt - 1) * d.stride_out_colsum + (x3p_row_tiles(M, N, bt) - 1) * d.ld_out_colsum + N, True)
    fwd = int(d.epilogue) == EPI_BIAS_ACT and int(d.activation) == ACT_RELU
    if d.relu_mask8 and (fwd or (int(d.epilogue) == EPI_RELU_GRAD and not d.aux)):
        add("relu_mask8", d.relu_mask8, 1, (bt - 1) * d.stride_mask8 + (M - 1) * d.ld_mask8 + (N + 7) // 8, fwd)
    return reg


def output_rects(d, kind):
    """The element rectangles a launch writes, per output: {name: (shape, strides, offset)} over the flat array at the pointer (for poisoning)."""
    M, N, bt, sp = int(d.M), int(d.N), int(d.batch), int(d.split_k)
    r = {"C": ((bt, sp, M, N), (d.stride_c, d.split_stride, d.ldc, 1), 0)}
    if d.C2 and int(d.epilogue) == EPI_BIAS_ACT and int(d.activation) >= ACT_SILU:
        r["C2"] = ((bt, 1, M, N), (d.stride_c2, 0, d.ldc2, 1), 0)
    if kind == "f32" and d.rowsum:
        r["rowsum"] = ((bt, sp, 1, M), (d.stride_rowsum, d.split_stride, 0, 1), 0)
    if kind == "x3p":
        if not d.C:
            del r["C"]
        if d.Cp:
            npl = 1 if int(d.planes) == 1 else 3
            r["Cp"] = ((npl, bt, M, _r8(N)), (d.c_plane_stride if npl == 3 else 0, d.stride_cp, d.ldcp, 1), 0)
        if d.out_colsum:
            r["out_colsum"] = ((bt, 1, x3p_row_tiles(M, N, bt), N), (d.stride_out_colsum, 0, d.ld_out_colsum, 1), 0)
    return r


# ------------------------------------------------------------------------------------------------------------------- judging a launch
def _gather(d, kind, name, flat):
    M, N, bt, sp = int(d.M), int(d.N), int(d.batch), int(d.split_k)
    if name == "C":
        return matrix(flat.double(), bt, d.stride_c, M, N, d.ldc, sp, d.split_stride)
    if name == "C2":
        return matrix(flat.double(), bt, d.stride_c2, M, N, d.ldc2)
    if name == "rowsum":
        return view(flat.double(), (bt, sp, 1, M), (d.stride_rowsum, d.split_stride, 0, 1))
    if name == "out_colsum":
        return view(flat.double(), (bt, 1, x3p_row_tiles(M, N, bt), N), (d.stride_out_colsum, 0, d.ld_out_colsum, 1))
    if name == "relu_mask":
        return mask_bits(flat, bt, int(d.stride_mask), M, N, int(d.ld_mask))
    if name == "relu_mask8":
        return mask8_bits(flat, bt, int(d.stride_mask8), M, N, int(d.ld_mask8))
    raise KeyError(name)


def judge(d, kind, mem, outs, ring=True, aggregate=True):
    """Check one launch.  kind: 'f32' (pulse_gemm_f32) or 'x3p'.  mem: the model's inputs (flat float64 values at each input pointer; masks
    as integer words / bytes); outs: the flat outputs at each output pointer after the launch (float32, int16 bf16 bits, int32 / uint8 masks).
    aggregate=False: the aggregate ratios are measured and returned but not held against RHO (see the fuzz test: at some shapes the product
    never issues, the device's fp32 matmul is far more accurate than any sequential fp32 accumulation).
    -> {"worst": max err / tol, "agg": max aggregate ratio (fp32-grade launches), "yard": max yardstick ratio, "problems": [str]}."""
    model = gemm_f32_model if kind == "f32" else (lambda dd, mm, yardstick=False: gemm_x3p_model(dd, mm, yardstick, ring))
    m_in = dict(mem)
    for k, v in outs.items():
        m_in.setdefault(k, v)
    exp = model(d, m_in)
    yard = model(d, m_in, yardstick=True) if any(e.fp32_grade for e in exp.values()) else {}
    rep = {"worst": 0.0, "agg": 0.0, "yard": 0.0, "problems": []}
    bad = rep["problems"]
    got = {}
    for name, e in exp.items():
        if name in ("relu_mask", "relu_mask8"):
            continue
        if name == "Cp":
            g = _cp_value(d, outs["Cp"], bad, got.get("C"))
        else:
            g = _gather(d, kind, name, outs[name])
        got[name] = g
        w = elementwise_ratio(g, e)
        rep["worst"] = max(rep["worst"], w)
        if not w <= 1.0:
            bad.append(f"{name}: worst err / tol {w:.3g}")
        if e.bf16:
            bad += [f"{name}: {p}" for p in bf16_output_problems(g, e)]
        if e.fp32_grade and name in yard:
            a = aggregate_ratio(g, e.R, yard[name].R)
            y = yardstick_ratio(yard[name].R, e.R, e.S)
            rep["agg"], rep["yard"] = max(rep["agg"], a), max(rep["yard"], y)
            if aggregate and not a <= 1.0:
                bad.append(f"{name}: rms error {a * RHO:.3g} x the fp32 yardstick's")
            if not y <= 1.0:
                bad.append(f"{name}: the yardstick is not fp32-grade (ratio {y:.3g})")
    if int(d.split_k) > 1:                            # the slab sum meets the bound of the full reduction
        e = exp["C"]
        s_err = (got["C"].sum(1) - e.R.sum(1)).abs()
        if bool((s_err > e.tol.sum(1)).any()) or bool(torch.isnan(s_err).any()):
            bad.append("C: the slab sum misses the full reduction")
        if "rowsum" in exp:
            r_err = (got["rowsum"].sum(1) - exp["rowsum"].R.sum(1)).abs()
            if bool((r_err > exp["rowsum"].tol.sum(1)).any()) or bool(torch.isnan(r_err).any()):
                bad.append("rowsum: the row sums over the slabs miss the full reduction")
    for mname in ("relu_mask", "relu_mask8"):
        if mname in exp and mname in outs:
            stored = got["C"][:, 0] if "C" in got else got["Cp"][:, 0]
            bad += [f"{mname}: {p}" for p in mask_problems(_gather(d, kind, mname, outs[mname]), stored, exp[mname])]
    if "out_colsum" in got:                           # ... and equal the column sums of what the launch stored (the bf16 matrix if there is one)
        stored = got["Cp"][:, 0] if ("Cp" in got and int(d.planes) == 1) or "C" not in got else got["C"][:, 0]
        tiles = got["out_colsum"].shape[2]
        h = 256 if tiles != (int(d.M) + 127) // 128 else 128
        st = torch.nn.functional.pad(stored, (0, 0, 0, tiles * h - int(d.M))).reshape(stored.shape[0], tiles, h, -1)
        lim = gamma(h) * st.abs().sum(2)
        if bool(((got["out_colsum"][:, 0] - st.sum(2)).abs() > lim).any()):
            bad.append("out_colsum: not the column sums of the stored output")
    return rep


def _cp_value(d, flat16, bad, stored_c):
    """(batch, 1, M, N) value of the Cp output planes; checks their exactness and the zero pad columns."""
    M, N, bt = int(d.M), int(d.N), int(d.batch)
    npl = 1 if int(d.planes) == 1 else 3
    full = [bf16_bits_to_f64(view(flat16, (bt, M, _r8(N)), (d.stride_cp, d.ldcp, 1), p * (d.c_plane_stride if npl == 3 else 0)))
            for p in range(npl)]
    if any(bool((f[..., N:] != 0).any()) for f in full):
        bad.append("Cp: pad columns [N, roundup8(N)) not zero")
    ps = [f[..., :N] for f in full]
    if npl == 1:
        if stored_c is not None and not torch.equal(ps[0], rne_bf16(stored_c[:, 0])):
            bad.append("Cp: not RNE_bf16 of the stored C")
        return ps[0][:, None]
    bad += [f"Cp: {p}" for p in planes_problems(ps[0], ps[1], ps[2], stored_c[:, 0] if stored_c is not None else None)]
    return (ps[0] + ps[1] + ps[2])[:, None]
