"""Tensor-level wrappers for the learner-side C-ABI entries (GEMM, normaliser, PPO loss, Adam ...).

Same rules as ``ops.py``: GPU tensors only, enqueue on torch's current stream, no fallback.
"""
import ctypes
import functools
import math
import os

import torch

from . import _lib
from ._lib import ACT_NONE, ACT_RELU, ACT_SILU, EPI_BIAS_ACT, GEMM_RED_CONTIG, GemmDesc, PpoLossArgs
from ._marshal import b16 as _b16, entry as _entry, launch as _launch, mask_u8 as _marshal_mask, ptr, rows2d, stream as _stream

ACTIVATIONS = {"None": ACT_NONE, "none": ACT_NONE, None: ACT_NONE, "relu": ACT_RELU, "silu": ACT_SILU}

# pointer of an optional tensor; given a name, the tensor is validated first (unit inner stride unless unit_stride=False).  In this module a
# tensor that is not on the GPU is a TypeError.
_p = functools.partial(ptr, unit_stride=True, not_gpu=TypeError)
_rows = functools.partial(rows2d, not_gpu=TypeError)
_I16, _I64, _F64 = torch.int16, torch.int64, torch.float64


class GemmProfiler:
    """Brackets every pulse_gemm_f32 launch with a HIP event pair on the launch stream (torch's
    current stream IS the stream the kernels are enqueued on) and tallies algorithmic FLOPs.
    Used by bench.py for the live roofline figure; off by default."""

    def __init__(self):
        self.enabled = False
        self.records = []          # (start_event, end_event, flops, tag)
        self._pool = []

    def start(self):
        self.enabled, self.records = True, []

    def stop(self):
        self.enabled = False

    def _event(self):
        return self._pool.pop() if self._pool else torch.cuda.Event(enable_timing=True)

    def summary(self):
        """-> dict tag -> (launches, seconds, flops); call after a synchronize."""
        out = {}
        for s, e, fl, tag in self.records:
            n, t, f = out.get(tag, (0, 0.0, 0.0))
            out[tag] = (n + 1, t + s.elapsed_time(e) * 1e-3, f + fl)
            self._pool += [s, e]
        self.records = []
        return out


PROFILER = GemmProfiler()

# How an fp32 GEMM is computed (inputs / outputs / storage are fp32 either way):
#   "x3"      three-way bf16 operand split, six bf16 MFMAs per k step, fp32 accumulation (PULSE_GEMM_COMPUTE_F32X3): fp32-grade
#             results on the bf16 matrix pipe, the fast path on gfx950
#   "mfma32"  v_mfma_f32_32x32x2_f32 (PULSE_GEMM_COMPUTE_F32)
F32_MODE = os.environ.get("PULSE_GEMM_F32", "x3")
if F32_MODE not in ("x3", "mfma32"):
    raise ValueError(f"PULSE_GEMM_F32 must be 'x3' or 'mfma32', not {F32_MODE!r}")


def make_gemm_desc(A, B, C, *, M, N, K, lda, ldb, ldc, a_layout=GEMM_RED_CONTIG, b_layout=GEMM_RED_CONTIG, bias=None,
                   activation=ACT_NONE, epilogue=EPI_BIAS_ACT, aux=None, ldaux=0, C2=None, ldc2=0, batch=1, stride_a=0,
                   stride_b=0, stride_c=0, stride_c2=0, stride_bias=0, stride_aux=0, split_k=1, split_stride=0,
                   a_off=0, b_off=0, c_off=0, bias_off=0, aux_off=0, c2_off=0, algo_k=None, algo_n=None, rowsum=None, rowsum_off=0,
                   stride_rowsum=0, compute_bf16=False, f32_mode=None, relu_mask=None, ld_mask=0, stride_mask=0, mask_off=0):
    """Build (descriptor, algorithmic FLOPs, variant tag) once; launch many times with launch_gemm.
    ``relu_mask``: int32 tensor (alloc_relu_mask) -- a relu forward records the sign bits there, a relu-grad launch with aux=None reads them
    (pulse_hip.h: pulse_gemm_desc.relu_mask); ld_mask / stride_mask / mask_off in 32-bit words."""
    d = GemmDesc()
    d.A, d.B, d.C = _p(A, off=a_off), _p(B, off=b_off), _p(C, off=c_off)
    d.C2, d.bias, d.aux = _p(C2, off=c2_off), _p(bias, off=bias_off), _p(aux, off=aux_off)
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc, d.ldc2, d.ldaux = lda, ldb, ldc, ldc2, ldaux
    d.a_layout, d.b_layout, d.batch = a_layout, b_layout, batch
    d.stride_a, d.stride_b, d.stride_c, d.stride_c2 = stride_a, stride_b, stride_c, stride_c2
    d.stride_bias, d.stride_aux = stride_bias, stride_aux
    d.split_k, d.split_stride, d.activation, d.epilogue = split_k, split_stride, activation, epilogue
    d.rowsum, d.stride_rowsum = _p(rowsum, off=rowsum_off), stride_rowsum
    if relu_mask is not None:
        if relu_mask.dtype != torch.int32:
            raise TypeError("relu_mask must be an int32 tensor (alloc_relu_mask)")
        d.relu_mask, d.ld_mask, d.stride_mask = _p(relu_mask, None, torch.int32, mask_off), int(ld_mask), int(stride_mask)
    # bf16 MFMA with fp32 storage (bf16 autocast over fp32 master weights); split-K slabs are partial sums and stay unrounded
    x3 = (not compute_bf16) and (f32_mode or F32_MODE) == "x3"
    d.compute_type = _lib.GEMM_COMPUTE_BF16 if compute_bf16 else (_lib.GEMM_COMPUTE_F32X3 if x3 else _lib.GEMM_COMPUTE_F32)
    d.round_output_bf16 = 1 if (compute_bf16 and split_k == 1) else 0
    tag = ("fwd" if b_layout == GEMM_RED_CONTIG else "dx") if a_layout == GEMM_RED_CONTIG else "dw"
    if compute_bf16:
        tag = "bf16_" + tag
    elif x3:
        tag = "x3_" + tag
    flops = 2.0 * M * (algo_n if algo_n else N) * (algo_k if algo_k else K) * batch
    return d, flops, tag


def alloc_relu_mask(rows, cols, device):
    """The ReLU bit mask of a (rows, cols) activation matrix (pulse_gemm_desc.relu_mask): (roundup64(rows) / 8, roundup4(cols) / 4) int32,
    ld_mask = its row pitch in words.  1 bit per activation: 1/32 of the fp32 matrix a relu-grad epilogue would otherwise re-read."""
    return torch.zeros((rows + 63) // 64 * 8, (cols + 3) // 4, dtype=torch.int32, device=device)


def alloc_relu_mask8(rows, cols, device):
    """The ReLU bit mask of a (rows, cols) activation matrix in the planar kernels' layout (pulse_gemm_x3p_desc.relu_mask8): one byte per row
    and 8 columns."""
    return torch.zeros(rows, (cols + 7) // 8, dtype=torch.uint8, device=device)


def dw_split(tiles, max_split, fill=512):
    """Batch-split of a weight-gradient GEMM: the smallest power-of-two fraction of ``max_split`` (the slab count of the gradient
    buffer) that still gives ``fill`` workgroups = two per CU.  Fewer, longer reductions amortise each workgroup's prologue /
    epilogue (measured on the layer-1 dW of cfg2: 4 slabs 386 us, 8 slabs 404 us, 16 slabs 436 us); the slabs a layer does not
    write stay zero (allocated zeroed, never touched), so the ordered slab reduce is unchanged."""
    s = max_split
    while s > 1 and s % 2 == 0 and tiles * (s // 2) >= fill:
        s //= 2
    return s


def x3_tile_costs(M, N, z, k=16384):
    """(narrow, wide) cost of an x3 launch with z = batch x split_k grid slices, in the launcher's units (gemm_api.hip: x3_wide_tile): one
    128 x 128 tile alone on a CU = 1.5 per unit of reduction length, two sharing a CU 2; a 256 x 256 workgroup has a CU to itself at about
    3.3 (more on short reductions, whose prologue / epilogue nothing hides)."""
    nt = ((M + 127) // 128) * ((N + 127) // 128) * z
    wt = ((M + 255) // 256) * ((N + 255) // 256) * z
    rem = nt % 512
    narrow = 2.0 * (nt // 512) + (0.0 if rem == 0 else 1.5 if rem <= 256 else 2.0)       # a lone workgroup is not twice as fast as a paired one
    wide_round = 2.0 * (0.1526 * k + 8.0) / (0.0924 * k + 5.0)          # k = the reduction length one workgroup walks (plain epilogue)
    wide = wide_round * ((wt + 255) // 256) if (M > 128 and N > 128) else float("inf")
    return narrow, wide


def dw_split_x3(M, N, batch, max_split, K=16384):
    """Slab count of an fp32 (x3) weight-gradient launch now that the launcher has two tilings: the power-of-two fraction of ``max_split`` with
    the lowest modelled time = min(narrow, wide cost) / split (the reduction length per workgroup is K / split) plus a charge per slab for its
    write and its share of the reduce (calibrated on the 2048 x 960 output: 16 us per 4 slabs against 281 us of GEMM), fewer slabs on ties.  cfg2 layer 1 (2048 x 960): 4 slabs on the narrow tiling -> 8 on the wide one
    (327 -> 296 us, profiles/r05_gemm_x3_wide_ab.txt); the [512, 1024] pair keeps 8 narrow slabs."""
    # the tiling the LAUNCHER will use (environment switch read once by the library + this thread's gemm option 4): planner and launcher
    # cannot disagree (round-5 advisor finding)
    if F32_MODE != "x3" or _lib.load().pulse_gemm_x3_mode() == 1:
        return dw_split(((M + 127) // 128) * ((N + 127) // 128) * batch, max_split)
    best, best_t = max_split, None
    s = max_split
    while s >= 1:
        t = min(x3_tile_costs(M, N, batch * s, max(16, K // s))) / s + 0.006 * s * (M * N * batch) / (2048.0 * 960.0)      # + the slab's write and its share of the reduce
        if best_t is None or t < best_t - 1e-9 or abs(t - best_t) <= 1e-9:
            best, best_t = s, t
        if s % 2:
            break
        s //= 2
    return best


def dw_split_b16(M, N, batch, max_split):
    """Slab count of a bf16-storage weight-gradient launch (pulse_gemm_x3p, planes = 1, both operands [red][out]).  The 256 x 256 tile moves
    2/3 of the bytes per MFMA of the 256 x 128 one (profiles/r04_ab_runs.txt: 2048 x 934 over 16384 rows: 124 us on 64 narrow tiles x 4
    slabs, 87 us on 32 wide tiles x 8 slabs), so when the wide tiling fills the chip within ``max_split`` slabs its count is returned -- the
    launcher's own rule (a wide workgroup must not cost a round) then picks that tile; otherwise the narrow tiling's count."""
    tm = (M + 255) // 256
    tw = tm * ((N + 255) // 256) * batch
    sw = dw_split(tw, max_split, fill=256)
    if N > 128 and tw * sw >= 192:
        return sw
    return dw_split(tm * ((N + 127) // 128) * batch, max_split, fill=256)


def _launch_desc(name, d, flops, tag, stream, retag=None):
    """One GEMM launch of entry ``name``; with the profiler on, bracketed by an event pair and recorded under ``tag`` (``retag(tag)``, asked
    after the launch, when the entry can say more about what served it)."""
    if not PROFILER.enabled:
        return _launch(name, ctypes.byref(d), st=stream)
    ev0, ev1 = PROFILER._event(), PROFILER._event()
    ev0.record()
    _launch(name, ctypes.byref(d), st=stream)
    ev1.record()
    PROFILER.records.append((ev0, ev1, flops, retag(tag) if retag else tag))


def _x3w_tag(tag):
    """An x3 launch served by the 256 x 256 tile (gemm_x3w_kernel) gets its own line in the bench's roofline."""
    return "x3w_" + tag[3:] if tag.startswith("x3_") and _entry("pulse_gemm_last_tile")() == 256 else tag


def launch_gemm(d, flops=0.0, tag="fwd", stream=None):
    _launch_desc("pulse_gemm_f32", d, flops, tag, stream, _x3w_tag)


def gemm(A, B, C, **kw):
    """C[m][n] = epilogue(sum_k A(m,k) B(n,k)).  A/B/C/... are tensors used only as base pointers
    (+ *_off floats); all geometry is explicit (pitches in floats)."""
    launch_gemm(*make_gemm_desc(A, B, C, **kw))


class Plan:
    """A pre-built launch sequence: GEMM descriptors and bound C-ABI calls are created once per
    workspace, so replaying a forward / backward pass costs one ctypes call per kernel."""

    # op kinds: ops holds (kind, descriptor, flops, tag) for the two GEMM kinds and (kind, bound entry, arguments, entry name) for the others
    GEMM, CALL, GEMM_X3P, PARTIAL_REDUCE = 0, 1, 2, 3

    def __init__(self, bf16=False):
        self.ops = []
        self.split = 0
        self.bf16 = bool(bf16)          # every GEMM of this plan runs on the bf16 MFMA (mixed_precision training passes)
        self.partial_reduces = []       # (dst_off, count, rows, src) of every call_partial_reduce

    def gemm(self, A, B, C, **kw):
        kw.setdefault("compute_bf16", self.bf16)
        self.ops.append((Plan.GEMM,) + make_gemm_desc(A, B, C, **kw))

    def call(self, name, *args):
        self.ops.append((Plan.CALL, _entry(name), args, name))     # (the tuple keeps ctypes arrays among the arguments alive)

    def call_partial_reduce(self, src, rows, count, slabs, dst_off):
        """Ordered sum of ``rows`` partial rows of ``src`` (row stride src.stride(0), ``count`` floats each) into slab 0 of ``slabs`` at element
        ``dst_off`` (pulse_reduce_slabs).  Registered separately: run(skip_partial_reduces=True) leaves these launches out when the caller's
        ReduceGrads reads the partials itself (``partial_reduces`` lists what it has to read)."""
        name = "pulse_reduce_slabs"
        self.ops.append((Plan.PARTIAL_REDUCE, _entry(name), (src.data_ptr(), int(rows), int(src.stride(0)), int(count), _p(slabs, off=int(dst_off)), 1.0), name))
        self.partial_reduces.append((int(dst_off), int(count), int(rows), src))

    def gemm_x3p(self, A, B, **kw):
        self.ops.append((Plan.GEMM_X3P,) + make_gemm_x3p_desc(A, B, **kw))

    def gemm_b16(self, A, B, **kw):
        """bf16-storage GEMM (pulse_gemm_x3p, planes = 1): A / B / Cp / aux are int16 (bf16 bit pattern) tensors."""
        self.gemm_x3p(A, B, planes=1, **kw)

    def refresh_b16(self, flat, flat16, count):
        """flat16[i] = bf16(flat[i]) for the whole flat parameter buffer: the bf16 weight image the plan's GEMMs read is rebuilt inside the
        plan, so no writer of the parameters (optimiser step, checkpoint load, broadcast, a test poking the buffer) can leave it stale."""
        n8 = (count + 7) // 8 * 8
        if flat16.dtype != torch.int16 or flat16.numel() < n8 or flat.numel() < count:
            raise ValueError("refresh_b16: flat16 must be an int16 buffer of roundup8(count) elements")
        self.call("pulse_split_planes", flat.data_ptr(), count, 1, count, flat16.data_ptr(), 0, n8, 0, None)

    def weights_b16(self, flat, flat16, count, transposes=()):
        """refresh_b16 + up to four transpose_b16 in ONE launch (pulse_weights_to_b16); ``transposes``: dicts with the keyword arguments of
        transpose_b16 plus ``x`` / ``out``."""
        n8 = (count + 7) // 8 * 8
        if flat16.dtype != torch.int16 or flat16.numel() < n8 or flat.numel() < count:
            raise ValueError("weights_b16: flat16 must be an int16 buffer of roundup8(count) elements")
        if len(transposes) > 4:
            raise ValueError("weights_b16: at most four transposes per launch")
        arr = (_lib.B16Transpose * max(1, len(transposes)))()
        for d, kw in zip(arr, transposes):
            d.in_, d.ld_in, d.rows, d.cols = _p(kw["x"], off=kw.get("x_off", 0)), kw["ld_in"], kw["rows"], kw["cols"]
            d.out, d.ld_out = _b16(kw["out"], "weights_b16: a transposed image", kw.get("out_off", 0)), kw["ld_out"]
            d.batch, d.stride_in, d.stride_out = kw.get("batch", 1), kw.get("stride_in", 0), kw.get("stride_out", 0)
        self.call("pulse_weights_to_b16", flat.data_ptr(), count, flat16.data_ptr(), len(transposes), arr)

    def transpose_b16(self, x, out, **kw):
        self.call("pulse_transpose_to_b16", _p(x, off=kw.pop("x_off", 0)), kw["ld_in"], kw["rows"], kw["cols"],
                  _b16(out, "transpose_b16: out", kw.pop("out_off", 0)), kw["ld_out"], kw.get("batch", 1), kw.get("stride_in", 0), kw.get("stride_out", 0))

    def colsum_b16(self, x, m, n, ld, slabs, num_slabs, slab_stride, out_off, x_off=0):
        """Bias gradient of a bf16 gradient matrix (m, n): slab s of ``slabs`` receives, at [out_off, out_off + n), the column sums over the
        s-th of ``num_slabs`` row ranges -- summed with the weight gradients by the one slab reduce, like the fp32 kernels' ``rowsum``."""
        self.call("pulse_colsum_partial_b16", _b16(x, "colsum_b16: x", x_off), m, n, ld, num_slabs, _p(slabs, off=out_off), slab_stride)

    def colsum_weighted_b16(self, x, w16, w_stride, m, n, ld, slabs, num_slabs, slab_stride, out_off, w_off=0):
        """slab s [out_off, out_off + n) = sum over the s-th row range of w16[m * w_stride] * x[m][:]: the weight gradient of a one-output Linear."""
        self.call("pulse_colsum_weighted_b16", _b16(x, "colsum_weighted_b16: x"), m, n, ld, _b16(w16, "colsum_weighted_b16: w16", w_off), w_stride,
                  num_slabs, _p(slabs, off=out_off), slab_stride)

    def run(self, start=0, stop=None, skip_partial_reduces=False):
        """``skip_partial_reduces``: leave out the small ordered reduces registered with call_partial_reduce -- the caller's fused gradient reduce
        (ReduceGrads regions with their own source) sums those partials itself.
        (Round 5 measured replaying plan segments as captured HIP graphs: flat inside the epoch -- cfg2 68.0 / 68.6 ms eager vs 68.4 / 69.2,
        profiles/r05_ab_runs.txt; the update is one dependent chain the host enqueues far ahead of the device.  The path was removed in round 6.)"""
        st = _stream()
        GEMM, GEMM_X3P, CALL, check = self.GEMM, self.GEMM_X3P, self.CALL, _lib.check
        for kind, what, args, tag in self.ops[start:stop]:
            if kind == GEMM:
                launch_gemm(what, args, tag, st)
            elif kind == GEMM_X3P:
                launch_gemm_x3p(what, args, tag, st)
            elif kind == CALL or not skip_partial_reduces:
                check(what(*args, st), tag)


# --------------------------------------------------------------------------- #
# PULSE VAE head algebra (include/pulse_hip.h section 4c)
# --------------------------------------------------------------------------- #
# The three launches in the shipped form -- learned prior, Gaussian posterior -- keep their signatures; ``*_modes`` below take the prior /
# posterior variants as further keywords whose defaults are that form (one C entry each: a zeroed mode field is the shipped form).
PRIOR_LEARNED, PRIOR_FIXED, PRIOR_NONE = 0, 1, 2           # PULSE_VAE_PRIOR_* (pulse_hip.h)


def vae_embed(heads, x, ain, *, rows, embedding_size, self_obs_size, z_col, eps=None, cin=None, clamp=True, clamp_max=2.0):
    vae_embed_modes(heads, x, ain, rows=rows, embedding_size=embedding_size, self_obs_size=self_obs_size, z_col=z_col, eps=eps, cin=cin, clamp=clamp,
                    clamp_max=clamp_max)


def vae_kin_loss(pred, gt, zheads, pheads, progress, dmu, partials, *, rows, num_actions, embedding_size, horizon, clamp=True, clamp_max=2.0,
                 use_ar1=True, use_regu=False):
    vae_kin_loss_modes(pred, gt, zheads, pheads, progress, dmu, partials, rows=rows, num_actions=num_actions, embedding_size=embedding_size,
                       horizon=horizon, clamp=clamp, clamp_max=clamp_max, use_ar1=use_ar1, use_regu=use_regu)


def vae_head_backward(zheads, dzheads, *, rows, embedding_size, horizon=1, pheads=None, dpheads=None, eps=None, dz=None, progress=None, clamp=True,
                      clamp_max=2.0, c_kl=0.0, c_ar1=0.0, c_regu=0.0):
    vae_head_backward_modes(zheads, dzheads, rows=rows, embedding_size=embedding_size, horizon=horizon, pheads=pheads, dpheads=dpheads, eps=eps, dz=dz,
                            progress=progress, clamp=clamp, clamp_max=clamp_max, c_kl=c_kl, c_ar1=c_ar1, c_regu=c_regu)


def vae_embed_modes(heads, x, ain, *, rows, embedding_size, self_obs_size, z_col, eps=None, cin=None, clamp=True, clamp_max=2.0,
                    sphere_posterior=False, embedding_norm=1.0):
    """vae_embed with the posterior mode: ``sphere_posterior`` writes project_to_norm(z, embedding_norm) (embedding_size <= 32)."""
    a = _lib.VaeEmbedArgs()
    a.heads, a.heads_stride = _p(heads, "heads"), heads.stride(0)
    a.eps, a.eps_stride = _p(eps, "eps"), (eps.stride(0) if eps is not None else 0)
    a.x, a.x_stride = _p(x, "x"), x.stride(0)
    a.ain, a.ain_stride = _p(ain, "ain"), ain.stride(0)
    a.cin, a.cin_stride = _p(cin, "cin"), (cin.stride(0) if cin is not None else 0)
    a.rows, a.embedding_size, a.self_obs_size, a.z_col = rows, embedding_size, self_obs_size, z_col
    a.clamp_logvar, a.clamp_max = int(bool(clamp)), float(clamp_max)
    a.sphere_posterior, a.embedding_norm = int(bool(sphere_posterior)), float(embedding_norm)
    _launch("pulse_vae_embed", ctypes.byref(a))


def vae_embed_prior(pheads, x, ain, *, rows, embedding_size, self_obs_size, z_col, eps=None, cin=None, z_out=None, prior_mode=PRIOR_LEARNED,
                    prior_fixed_logvar=0.0, clamp=True, clamp_max=2.0, logvar_override=None, sphere_prior=False, sphere_posterior=False,
                    embedding_norm=1.0):
    """The generation step (form_embedding under flags.debug, amp_network_z_builder.py:101-119): z drawn from the prior into ``ain`` beside
    the self observation, as vae_embed lays it out.  ``pheads`` as vae_kin_loss_modes takes them (None with PRIOR_NONE, where z = eps);
    ``eps`` None: z = the prior mean; ``logvar_override``: a constant log-variance instead of the prior's; ``z_out``: (rows, E), z again."""
    a = _lib.VaeEmbedPriorArgs()
    a.pheads, a.pheads_stride = _p(pheads, "pheads"), (pheads.stride(0) if pheads is not None else 0)
    a.eps, a.eps_stride = _p(eps, "eps"), (eps.stride(0) if eps is not None else 0)
    a.x, a.x_stride = _p(x, "x"), x.stride(0)
    a.ain, a.ain_stride = _p(ain, "ain"), ain.stride(0)
    a.cin, a.cin_stride = _p(cin, "cin"), (cin.stride(0) if cin is not None else 0)
    a.z_out, a.z_out_stride = _p(z_out, "z_out"), (z_out.stride(0) if z_out is not None else 0)
    a.rows, a.embedding_size, a.self_obs_size, a.z_col = rows, embedding_size, self_obs_size, z_col
    a.prior_mode, a.prior_fixed_logvar = int(prior_mode), float(prior_fixed_logvar)
    a.clamp_logvar, a.clamp_max = int(bool(clamp)), float(clamp_max)
    a.logvar_override, a.logvar_override_value = int(logvar_override is not None), float(logvar_override or 0.0)
    a.sphere_prior, a.sphere_posterior, a.embedding_norm = int(bool(sphere_prior)), int(bool(sphere_posterior)), float(embedding_norm)
    _launch("pulse_vae_embed_prior", ctypes.byref(a))


def vae_project(a, out, *, rows, cols, norm, b=None):
    """out = project_to_norm(a [+ b], norm) row by row (phc/utils/torch_utils.py:38-43); cols <= 32."""
    _launch("pulse_vae_project", _p(a, "a"), a.stride(0), _p(b, "b"), (b.stride(0) if b is not None else 0), _p(out, "out"), out.stride(0),
            rows, cols, float(norm))


def vae_kin_loss_modes(pred, gt, zheads, pheads, progress, dmu, partials, *, rows, num_actions, embedding_size, horizon, clamp=True, clamp_max=2.0,
                       use_ar1=True, use_regu=False, prior_mode=PRIOR_LEARNED, prior_fixed_logvar=0.0, sphere_prior=False, embedding_norm=1.0):
    """``pheads``: (rows, 2E) [mu | logvar] with PRIOR_LEARNED, (rows, E) with PRIOR_FIXED, None with PRIOR_NONE."""
    a = _lib.VaeKinArgs()
    a.pred, a.pred_stride, a.gt, a.gt_stride = _p(pred, "pred"), pred.stride(0), _p(gt, "gt"), gt.stride(0)
    a.zheads, a.zheads_stride = _p(zheads, "zheads"), zheads.stride(0)
    a.pheads, a.pheads_stride = _p(pheads, "pheads"), (pheads.stride(0) if pheads is not None else 0)
    a.progress = _p(progress, "progress", torch.int64)
    a.rows, a.num_actions, a.embedding_size, a.horizon = rows, num_actions, embedding_size, horizon
    a.clamp_logvar, a.clamp_max, a.use_ar1, a.use_regu = int(bool(clamp)), float(clamp_max), int(bool(use_ar1)), int(bool(use_regu))
    a.dmu, a.dmu_stride = _p(dmu, "dmu"), dmu.stride(0)
    a.partials, a.num_blocks = _p(partials, "partials"), partials.shape[0]
    a.prior_mode, a.prior_fixed_logvar = int(prior_mode), float(prior_fixed_logvar)
    a.sphere_prior, a.embedding_norm = int(bool(sphere_prior)), float(embedding_norm)
    _launch("pulse_vae_kin_loss", ctypes.byref(a))


def vae_head_backward_modes(zheads, dzheads, *, rows, embedding_size, horizon=1, pheads=None, dpheads=None, eps=None, dz=None, progress=None, clamp=True,
                            clamp_max=2.0, c_kl=0.0, c_ar1=0.0, c_regu=0.0, prior_mode=PRIOR_LEARNED, prior_fixed_logvar=0.0, sphere_prior=False,
                      sphere_posterior=False, embedding_norm=1.0):
    a = _lib.VaeHeadBwdArgs()
    a.zheads, a.zheads_stride = _p(zheads, "zheads"), zheads.stride(0)
    a.pheads, a.pheads_stride = _p(pheads, "pheads"), (pheads.stride(0) if pheads is not None else 0)
    a.eps, a.eps_stride = _p(eps, "eps"), (eps.stride(0) if eps is not None else 0)
    a.dz, a.dz_stride = _p(dz, "dz"), (dz.stride(0) if dz is not None else 0)
    a.progress = _p(progress, "progress", torch.int64)
    a.rows, a.embedding_size, a.horizon = rows, embedding_size, horizon
    a.clamp_logvar, a.clamp_max = int(bool(clamp)), float(clamp_max)
    a.c_kl, a.c_ar1, a.c_regu = float(c_kl), float(c_ar1), float(c_regu)
    a.dzheads, a.dzheads_stride = _p(dzheads, "dzheads"), dzheads.stride(0)
    a.dpheads, a.dpheads_stride = _p(dpheads, "dpheads"), (dpheads.stride(0) if dpheads is not None else 0)
    a.prior_mode, a.prior_fixed_logvar = int(prior_mode), float(prior_fixed_logvar)
    a.sphere_prior, a.sphere_posterior, a.embedding_norm = int(bool(sphere_prior)), int(bool(sphere_posterior)), float(embedding_norm)
    _launch("pulse_vae_head_backward", ctypes.byref(a))


# --------------------------------------------------------------------------- #
# MCP composer head (include/pulse_hip.h section 4e)
# --------------------------------------------------------------------------- #
def mcp_head_forward(h, mu, *, rows, num_prim):
    """mu[:, :num_prim] = softmax(h[:, :num_prim], dim=1): the nn.Softmax AMPMCPBuilder appends to the composer (amp_network_mcp_builder.py:53-55)."""
    hp, hs = _rows(h, "h", rows, num_prim)
    mp, ms = _rows(mu, "mu", rows, num_prim)
    _launch("pulse_mcp_head_forward", hp, hs, rows, num_prim, mp, ms)
    return mu


def mcp_head_backward(dmu, dz, *, rows, num_prim, mu=None, aux=None, activation=ACT_NONE):
    """dz = (softmax backward of dmu when ``mu`` is given, else dmu) * act'(.) with the derivative taken from ``aux`` (ACT_RELU: the activated
    output; ACT_SILU: the pre-activation; ACT_SILU_D: the stored derivative): the composer's tail down to its last Linear's output."""
    if activation != ACT_NONE and aux is None:
        raise ValueError("mcp_head_backward: the activation's derivative needs aux")
    dp, ds = _rows(dmu, "dmu", rows, num_prim)
    zp, zs = _rows(dz, "dz", rows, num_prim)
    mp, ms = _rows(mu, "mu", rows, num_prim) if mu is not None else (None, 0)
    ap, as_ = _rows(aux, "aux", rows, num_prim) if aux is not None else (None, 0)
    _launch("pulse_mcp_head_backward", dp, ds, mp, ms, ap, as_, int(activation), rows, num_prim, zp, zs)
    return dz


# --------------------------------------------------------------------------- #
# reference-motion records from raw clips (include/pulse_hip.h section 2b')
# --------------------------------------------------------------------------- #
def gaussian_weights(sigma=2.0, radius=8):
    """The weights scipy's gaussian_filter1d uses (scipy.ndimage._filters._gaussian_kernel1d, order 0), in double: |tap| = 0 .. radius."""
    import numpy as np
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return [float(v) for v in phi[radius:]]


def motion_build(frames, offsets, *, src_rot, src_trans, clip_src_start, clip_out_start, clip_frames, clip_dt, local_translation, parents,
                 clip_heading=None, clip_crop_start=None):
    """pulse_motion_build: fill ``frames`` (total, frame_stride), the packed records of ``MotionLib.record_layout``, from staged raw clips.
    Device tensors: ``src_rot`` (S, J, 4) / ``src_trans`` (S, 3) fp32, ``clip_src_start`` (M) / ``clip_out_start`` (M + 1) /
    ``clip_crop_start`` (M, optional) int64, ``clip_dt`` (M) / ``clip_heading`` (M, optional) / ``local_translation`` (M, J, 3) fp32.
    Host: ``clip_frames`` (M) int64 CPU tensor (validated by the launcher), ``parents`` a sequence of J ints."""
    a = _lib.MotionBuildArgs()
    for name, t, dt in (("src_rot", src_rot, torch.float32), ("src_trans", src_trans, torch.float32), ("clip_src_start", clip_src_start, torch.int64),
                        ("clip_crop_start", clip_crop_start, torch.int64), ("clip_out_start", clip_out_start, torch.int64), ("clip_dt", clip_dt, torch.float32),
                        ("clip_heading", clip_heading, torch.float32), ("local_translation", local_translation, torch.float32), ("frames", frames, torch.float32)):
        ptr = _p(t, name, dt)
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name}: contiguous tensor expected, got strides {tuple(t.stride())}")
        setattr(a, name, ptr)
    if not isinstance(clip_frames, torch.Tensor) or clip_frames.device.type != "cpu" or clip_frames.dtype != torch.int64 or not clip_frames.is_contiguous():
        raise TypeError("clip_frames: contiguous int64 CPU tensor expected (the launcher validates the frame counts on the host)")
    m, j = clip_frames.numel(), len(parents)
    if src_rot.dim() != 3 or tuple(src_rot.shape[1:]) != (j, 4) or tuple(src_trans.shape) != (src_rot.shape[0], 3):
        raise ValueError(f"src_rot / src_trans: expected (S, {j}, 4) and (S, 3), got {tuple(src_rot.shape)} and {tuple(src_trans.shape)}")
    for name, t, shape in (("clip_src_start", clip_src_start, (m,)), ("clip_crop_start", clip_crop_start, (m,)), ("clip_out_start", clip_out_start, (m + 1,)),
                           ("clip_dt", clip_dt, (m,)), ("clip_heading", clip_heading, (m,)), ("local_translation", local_translation, (m, j, 3))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
    if frames.dim() != 2:
        raise ValueError(f"frames: expected (total_frames, frame_stride), got {tuple(frames.shape)}")
    par = (ctypes.c_int32 * j)(*[int(p) for p in parents])
    a.src_frames, a.num_clips, a.num_bodies = src_rot.shape[0], m, j
    a.clip_frames_host, a.parent_indices_host = clip_frames.data_ptr(), ctypes.cast(par, ctypes.c_void_p)
    a.total_frames, a.frame_stride = frames.shape[0], frames.shape[1]
    a.off_gts, a.off_grs, a.off_lrs = offsets["gts"], offsets["grs"], offsets["lrs"]
    a.off_gvs, a.off_gavs, a.off_dvs = offsets["gvs"], offsets["gavs"], offsets["dvs"]
    a.filter_w[:] = gaussian_weights()
    _launch("pulse_motion_build", ctypes.byref(a))
    return frames


INGEST_MAX_BODIES = 32


def motion_ingest(out_rot, out_trans, *, src_pose, src_trans, clip_src_start, clip_skip, clip_frames, parents, joint_map, mirror_map=None,
                  clip_mirror=None, upright_start=True, root_offset=(0.0, 0.0, 0.0), out_pose_quat=None, out_pose_aa=None,
                  out_trans_orig=None):
    """pulse_motion_ingest: raw SMPL pose rows -> ``out_rot`` (T, J, 4) pose_quat_global and ``out_trans`` (T, 3) root_trans_offset, one launch
    (include/pulse_hip.h section 2b'.1).  Device tensors: ``src_pose`` (S, 72) / ``src_trans`` (S, 3) fp32 and the outputs.  Host: the
    per-clip tables ``clip_src_start`` / ``clip_skip`` / ``clip_frames`` (M) int64 CPU tensors and ``clip_mirror`` (M) bool / uint8, optional (the
    launcher validates them; their device copies are made here), ``parents`` / ``joint_map`` / ``mirror_map`` sequences of J ints."""
    a = _lib.MotionIngestArgs()
    for name, t in (("src_pose", src_pose), ("src_trans", src_trans), ("out_rot", out_rot), ("out_trans", out_trans), ("out_pose_quat", out_pose_quat),
                    ("out_pose_aa", out_pose_aa), ("out_trans_orig", out_trans_orig)):
        ptr = _p(t, name, torch.float32)
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name}: contiguous tensor expected, got strides {tuple(t.stride())}")
        setattr(a, name, ptr)
    for name, t in (("clip_src_start", clip_src_start), ("clip_skip", clip_skip), ("clip_frames", clip_frames)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cpu" or t.dtype != torch.int64 or not t.is_contiguous() or t.dim() != 1:
            raise TypeError(f"{name}: contiguous (M) int64 CPU tensor expected (the launcher validates the clip tables on the host)")
    m, j = clip_frames.numel(), len(parents)
    if j > INGEST_MAX_BODIES:
        raise ValueError(f"motion_ingest: num_bodies {j} > {INGEST_MAX_BODIES} (one lane of a half-wave per body)")
    if clip_src_start.numel() != m or clip_skip.numel() != m:
        raise ValueError(f"clip_src_start / clip_skip: expected shape ({m},)")
    if src_pose.dim() != 2 or src_pose.shape[1] != 72 or tuple(src_trans.shape) != (src_pose.shape[0], 3):
        raise ValueError(f"src_pose / src_trans: expected (S, 72) and (S, 3), got {tuple(src_pose.shape)} and {tuple(src_trans.shape)}")
    total, dev = int(clip_frames.sum()), out_rot.device
    for name, t, shape in (("out_rot", out_rot, (total, j, 4)), ("out_trans", out_trans, (total, 3)), ("out_pose_quat", out_pose_quat, (total, j, 4)),
                           ("out_pose_aa", out_pose_aa, (total, 72)), ("out_trans_orig", out_trans_orig, (total, 3))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
    if len(joint_map) != j or (mirror_map is not None and len(mirror_map) != j):
        raise ValueError(f"joint_map / mirror_map: {j} entries expected, one per body")
    out_start = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(clip_frames, 0)])
    keep = [clip_src_start.to(dev), clip_skip.to(dev), out_start.to(dev)]
    a.clip_src_start, a.clip_skip, a.clip_out_start = (t.data_ptr() for t in keep)
    if clip_mirror is not None:
        if clip_mirror.numel() != m:
            raise ValueError(f"clip_mirror: expected shape ({m},)")
        keep.append(clip_mirror.to(torch.uint8).contiguous().to(dev))
        a.clip_mirror = keep[-1].data_ptr()
    par = (ctypes.c_int32 * j)(*[int(p) for p in parents])
    a.clip_src_start_host, a.clip_skip_host, a.clip_frames_host = clip_src_start.data_ptr(), clip_skip.data_ptr(), clip_frames.data_ptr()
    a.parent_indices_host = ctypes.cast(par, ctypes.c_void_p)
    a.src_frames, a.num_clips, a.num_bodies = src_pose.shape[0], m, j
    a.joint_map[:j] = [int(v) for v in joint_map]
    a.mirror_map[:j] = [int(v) for v in mirror_map] if mirror_map is not None else list(range(j))
    a.upright_start, a.total_frames = int(bool(upright_start)), total
    a.root_offset[:] = [float(v) for v in root_offset]
    _launch("pulse_motion_ingest", ctypes.byref(a))
    return out_rot, out_trans


SMOOTH_MAX_RADIUS = 12
# convert_data_mdm.py:54: Rotation.from_euler('xyz', [pi / 2, 0, 0]) as scipy holds it, xyzw
MDM_ROOT_QUAT = (math.sin(math.pi / 4), 0.0, 0.0, math.cos(math.pi / 4))


def gaussian_taps(sigma, radius=None):
    """The weights of scipy's gaussian_filter1d(sigma) (scipy.ndimage._filters._gaussian_kernel1d, order 0) in double, |tap| = 0 .. radius;
    ``radius`` defaults to gaussian_filter1d's int(4 sigma + 0.5).  More than SMOOTH_MAX_RADIUS taps a side are refused."""
    import numpy as np
    sigma = float(sigma)
    if not math.isfinite(sigma) or sigma <= 0:
        raise ValueError(f"gaussian_taps: sigma {sigma} is not a positive finite number")
    radius = int(4.0 * sigma + 0.5) if radius is None else int(radius)
    if radius < 0 or radius > SMOOTH_MAX_RADIUS:
        raise ValueError(f"gaussian_taps: radius {radius} (sigma {sigma}) not in [0,{SMOOTH_MAX_RADIUS}]: pulse_motion_smooth holds {SMOOTH_MAX_RADIUS} taps a side")
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return [float(v) for v in phi[radius:]]


def quat_matrix(q):
    """scipy Rotation.as_matrix of a unit quaternion xyzw, row-major in double."""
    x, y, z, w = (float(v) for v in q)
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    return [x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw), 2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw), 2 * (xz - yw), 2 * (yz + xw),
            -x2 - y2 + z2 + w2]


def _clip_table(what, clip_frames, dev):
    if not isinstance(clip_frames, torch.Tensor) or clip_frames.device.type != "cpu" or clip_frames.dtype != _I64 or not clip_frames.is_contiguous() \
            or clip_frames.dim() != 1:
        raise TypeError(f"{what}: clip_frames: contiguous (M) int64 CPU tensor expected (the launcher validates the clip table on the host)")
    start = torch.cat([torch.zeros(1, dtype=_I64), torch.cumsum(clip_frames, 0)])
    return start.to(dev), int(clip_frames.sum())


def motion_euler_pose(out_pose, out_trans, *, src_theta, src_trans, clip_frames, floor_height=0.92, root_quat=MDM_ROOT_QUAT):
    """pulse_motion_euler_pose: per-joint Euler 'XYZ' angles in degrees ``src_theta`` (T, 72) and ``src_trans`` (T, 3) of packed clips ->
    ``out_pose`` (T, 72) axis-angle rows and ``out_trans`` (T, 3), the staging rows ``motion_ingest`` reads (include/pulse_hip.h section
    2b'.1a).  Host: ``clip_frames`` (M) int64 CPU tensor."""
    a = _lib.MotionEulerPoseArgs()
    for name, t in (("src_theta", src_theta), ("src_trans", src_trans), ("out_pose", out_pose), ("out_trans", out_trans)):
        ptr = _p(t, name, torch.float32)
        if not t.is_contiguous():
            raise ValueError(f"{name}: contiguous tensor expected, got strides {tuple(t.stride())}")
        setattr(a, name, ptr)
    start, total = _clip_table("motion_euler_pose", clip_frames, out_pose.device)
    for name, t, shape in (("src_theta", src_theta, (total, 72)), ("src_trans", src_trans, (total, 3)), ("out_pose", out_pose, (total, 72)),
                           ("out_trans", out_trans, (total, 3))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
    a.total_frames, a.num_clips = total, clip_frames.numel()
    a.clip_start, a.clip_frames_host = start.data_ptr(), clip_frames.data_ptr()
    a.root_quat[:] = [float(v) for v in root_quat]
    a.trans_matrix[:] = quat_matrix(root_quat)
    a.floor_height = float(floor_height)
    _launch("pulse_motion_euler_pose", ctypes.byref(a))
    return out_pose, out_trans


def motion_smooth(out_rot, out_trans, *, in_rot, in_trans, clip_frames, parents, sigma_rot=2.0, sigma_trans=3.0, out_pose_quat=None, sign_words=None):
    """pulse_motion_smooth: quat_correct along every clip, gaussian_filter1d(sigma_rot) of the corrected globals ``in_rot`` (T, J, 4) and
    renormalisation -> ``out_rot``, their local rotations -> ``out_pose_quat``, gaussian_filter1d(sigma_trans) of ``in_trans`` (T, 3) ->
    ``out_trans`` (include/pulse_hip.h section 2b'.1a).  A sigma of 0 leaves that filter out.  Host: ``clip_frames`` (M) int64 CPU tensor,
    ``parents`` J ints.  ``sign_words``: (T) int32 workspace, allocated here when not given.  No output may overlap an input."""
    a = _lib.MotionSmoothArgs()
    for name, t in (("in_rot", in_rot), ("in_trans", in_trans), ("out_rot", out_rot), ("out_trans", out_trans), ("out_pose_quat", out_pose_quat)):
        ptr = _p(t, name, torch.float32)
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name}: contiguous tensor expected, got strides {tuple(t.stride())}")
        setattr(a, name, ptr)
    j = len(parents)
    if j > INGEST_MAX_BODIES:
        raise ValueError(f"motion_smooth: num_bodies {j} > {INGEST_MAX_BODIES} (one lane of a half-wave per body)")
    start, total = _clip_table("motion_smooth", clip_frames, out_rot.device)
    for name, t, shape in (("in_rot", in_rot, (total, j, 4)), ("in_trans", in_trans, (total, 3)), ("out_rot", out_rot, (total, j, 4)),
                           ("out_trans", out_trans, (total, 3)), ("out_pose_quat", out_pose_quat, (total, j, 4))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
    for out_name, o, in_name, i in (("out_rot", out_rot, "in_rot", in_rot), ("out_pose_quat", out_pose_quat, "in_rot", in_rot),
                                    ("out_pose_quat", out_pose_quat, "out_rot", out_rot), ("out_trans", out_trans, "in_trans", in_trans)):
        if o is not None and o.data_ptr() < i.data_ptr() + i.numel() * 4 and i.data_ptr() < o.data_ptr() + o.numel() * 4:
            raise ValueError(f"motion_smooth: {out_name} overlaps {in_name}: the filters read their neighbours' unfiltered values, no output may alias an input")
    if sign_words is None:
        sign_words = torch.empty(max(total, 1), dtype=torch.int32, device=out_rot.device)
    if sign_words.dtype != torch.int32 or sign_words.numel() < total or not sign_words.is_contiguous():
        raise ValueError(f"sign_words: contiguous int32 tensor of at least {total} words expected")
    a.sign_words = _p(sign_words, "sign_words", torch.int32)
    for which, sigma in (("rot", sigma_rot), ("trans", sigma_trans)):
        if float(sigma) == 0.0:
            setattr(a, "radius_" + which, -1)
            continue
        taps = gaussian_taps(sigma)
        setattr(a, "radius_" + which, len(taps) - 1)
        getattr(a, "w_" + which)[:len(taps)] = taps
    par = (ctypes.c_int32 * j)(*[int(p) for p in parents])
    a.total_frames, a.num_clips, a.num_bodies = total, clip_frames.numel(), j
    a.clip_start, a.clip_frames_host, a.parent_indices_host = start.data_ptr(), clip_frames.data_ptr(), ctypes.cast(par, ctypes.c_void_p)
    _launch("pulse_motion_smooth", ctypes.byref(a))
    return out_rot, out_trans


EXPORT_MAX_BODIES = 32


def motion_export(out_rot, out_trans, *, rb, seg_env, seg_t0, seg_frames, parents, joint_map, dof_pos=None, upright_start=True,
                  root_offset=(0.0, 0.0, 0.0), out_pose_quat=None, out_pose_aa=None, out_trans_orig=None, out_body_quat=None, out_dof_pos=None):
    """pulse_motion_export: a recording ``rb`` (T, N, J, 13) -> ``out_rot`` (F, J, 4) pose_quat_global and ``out_trans`` (F, 3) root_trans_offset of
    every frame of every segment, one launch (include/pulse_hip.h section 2b'.2).  ``rb`` and ``dof_pos`` (T, N, 3 (J - 1)) are read in place:
    any view with unit inner stride.  Host: the per-segment tables ``seg_env`` / ``seg_t0`` / ``seg_frames`` (M) int64 CPU tensors (the launcher
    validates them; their device copies are made here), ``parents`` / ``joint_map`` sequences of J ints.  The optional outputs are contiguous."""
    a = _lib.MotionExportArgs()
    for name, t in (("out_rot", out_rot), ("out_trans", out_trans), ("out_pose_quat", out_pose_quat), ("out_pose_aa", out_pose_aa),
                    ("out_trans_orig", out_trans_orig), ("out_body_quat", out_body_quat), ("out_dof_pos", out_dof_pos)):
        ptr = _p(t, name, torch.float32)
        if t is not None and not t.is_contiguous():
            raise ValueError(f"{name}: contiguous tensor expected, got strides {tuple(t.stride())}")
        setattr(a, name, ptr)
    for name, t in (("seg_env", seg_env), ("seg_t0", seg_t0), ("seg_frames", seg_frames)):
        if not isinstance(t, torch.Tensor) or t.device.type != "cpu" or t.dtype != torch.int64 or not t.is_contiguous() or t.dim() != 1:
            raise TypeError(f"{name}: contiguous (M) int64 CPU tensor expected (the launcher validates the segment tables on the host)")
    m, j = seg_frames.numel(), len(parents)
    if j > EXPORT_MAX_BODIES:
        raise ValueError(f"motion_export: num_bodies {j} > {EXPORT_MAX_BODIES} (one lane of a half-wave per body)")
    if seg_env.numel() != m or seg_t0.numel() != m:
        raise ValueError(f"seg_env / seg_t0: expected shape ({m},)")
    a.rb = _p(rb, "rb", torch.float32)
    if rb.dim() != 4 or tuple(rb.shape[2:]) != (j, 13):
        raise ValueError(f"rb: expected (T, N, {j}, 13), got {tuple(rb.shape)}")
    steps, envs = rb.shape[0], rb.shape[1]
    a.rb_stride_t, a.rb_stride_n, a.rb_stride_b = rb.stride(0), rb.stride(1), rb.stride(2)
    if dof_pos is not None:
        a.dof_pos = _p(dof_pos, "dof_pos", torch.float32)
        if tuple(dof_pos.shape) != (steps, envs, 3 * (j - 1)):
            raise ValueError(f"dof_pos: expected {(steps, envs, 3 * (j - 1))}, got {tuple(dof_pos.shape)}")
        a.dof_stride_t, a.dof_stride_n = dof_pos.stride(0), dof_pos.stride(1)
        if j == 1:
            # a single body has no joint: dof_pos is zero floats wide, torch gives an empty tensor no address, and the launcher would take the
            # null for "no dof_pos" and refuse out_body_quat.  No float of it is read at J = 1; the recording's address says "present".
            a.dof_pos = a.rb
    total, dev = int(seg_frames.sum()), out_rot.device
    for name, t, shape in (("out_rot", out_rot, (total, j, 4)), ("out_trans", out_trans, (total, 3)), ("out_pose_quat", out_pose_quat, (total, j, 4)),
                           ("out_pose_aa", out_pose_aa, (total, 3 * j)), ("out_trans_orig", out_trans_orig, (total, 3)),
                           ("out_body_quat", out_body_quat, (total, j, 4)), ("out_dof_pos", out_dof_pos, (total, 3 * (j - 1)))):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
    if len(joint_map) != j:
        raise ValueError(f"joint_map: {j} entries expected, one per body")
    out_start = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(seg_frames, 0)])
    keep = [seg_env.to(dev), seg_t0.to(dev), out_start.to(dev)]
    a.seg_env, a.seg_t0, a.seg_out_start = (t.data_ptr() for t in keep)
    par = (ctypes.c_int32 * j)(*[int(p) for p in parents])
    a.seg_env_host, a.seg_t0_host, a.seg_frames_host = seg_env.data_ptr(), seg_t0.data_ptr(), seg_frames.data_ptr()
    a.parent_indices_host = ctypes.cast(par, ctypes.c_void_p)
    a.num_steps, a.num_envs, a.num_bodies, a.num_segments = steps, envs, j, m
    a.joint_map[:j] = [int(v) for v in joint_map]
    a.upright_start, a.total_frames = int(bool(upright_start)), total
    a.root_offset[:] = [float(v) for v in root_offset]
    _launch("pulse_motion_export", ctypes.byref(a))
    return out_rot, out_trans


KEYPOINT_MAX_BODIES, KEYPOINT_MAX_HISTORY = 31, 64
# humanoid_im_mcp_demo.py:66: the lengths of the limbs body 1 .. 5 hang on (parents 0, 1, 2, 3, 0), float32 as the reference keeps them
KEYPOINT_MEAN_LIMB_LENGTHS = (0.1061, 0.3624, 0.4015, 0.1384, 0.1132)


def keypoint_taps(sigmas=(10.0, 5.0, 2.0), history=30, truncate=4.0):
    """The tap table of pulse_keypoint_push, (len(sigmas), H, H) float64 on the CPU (needs no device): row L - 1 of table k holds the L weights
    with which ``scipy.ndimage.gaussian_filter1d(x, sigmas[k], axis=0, mode="mirror", truncate=truncate)[-1]`` combines L samples, oldest first;
    the rest of the row is zero.  Tap t of the kernel (radius int(truncate * sigma + 0.5), weights exp(-t^2 / (2 sigma^2)) normalised) lands on
    index (L - 1 + t) mod 2 (L - 1), reflected into 0 .. L - 1; L = 1 gives weight 1.  Default order: root component 2, root components 0 / 1,
    body coordinates (humanoid_im_mcp_demo.py:278-284)."""
    import numpy as np
    h = int(history)
    if not 1 <= h <= KEYPOINT_MAX_HISTORY:
        raise ValueError(f"keypoint_taps: history {history!r} not in [1, {KEYPOINT_MAX_HISTORY}]")
    out = np.zeros((len(sigmas), h, h), dtype=np.float64)
    for k, sigma in enumerate(sigmas):
        sigma = float(sigma)
        if not sigma > 0:
            raise ValueError(f"keypoint_taps: sigma {sigma!r} must be positive")
        radius = int(float(truncate) * sigma + 0.5)
        t = np.arange(-radius, radius + 1)
        w = np.exp(-0.5 / (sigma * sigma) * t.astype(np.float64) ** 2)
        w = w / w.sum()
        out[k, 0, 0] = 1.0
        for length in range(2, h + 1):
            period = 2 * (length - 1)
            idx = (length - 1 + t) % period
            idx = np.where(idx > length - 1, period - idx, idx)
            np.add.at(out[k, length - 1], idx, w)
    return out


def keypoint_frame(frame="y_up"):
    """The 3 x 3 matrix pulse_keypoint_push applies last, float64: "y_up" = the reference's to_isaac_mat (humanoid_im_mcp_demo.py:56: the
    rotation by -pi / 2 about x, built as scipy builds it from the quaternion (sin(-pi / 4), 0, 0, cos(-pi / 4))); "sim" = identity (keypoints
    already in the simulator's z-up frame).  Needs no device."""
    import numpy as np
    if frame == "sim":
        return np.eye(3)
    if frame != "y_up":
        raise ValueError(f"keypoint frame {frame!r}: 'y_up' or 'sim'")
    x, w = np.sin(-np.pi / 4), np.cos(-np.pi / 4)
    x2, w2, xw = x * x, w * w, x * w
    return np.array([[x2 + w2, 0.0, 0.0], [0.0, -x2 + w2, -2 * xw], [0.0, 2 * xw, -x2 + w2]])


def keypoint_push(j3d, *, taps, root_ring, body_ring, count, prev_pos, pos, vel, joint_map, parents, raw=None, env_mask=None,
                  mean_limb_lengths=KEYPOINT_MEAN_LIMB_LENGTHS, frame=None, dt=1.0 / 30.0):
    """pulse_keypoint_push: one frame of keypoints ``j3d`` (N, J, 3) float32 -> ``pos`` / ``vel`` (N, J, 3) of the filtered reference, one launch
    (include/pulse_hip.h section 2b'.3).  ``j3d`` is read in place: any view with unit inner stride (env and joint strides are honoured).
    State, updated in place, all contiguous: ``root_ring`` (N, H, 3), ``body_ring`` (N, H, J, 3), ``count`` (N,) int32, ``prev_pos`` (N, J, 3).
    ``taps`` (3, H, H) float32 on the device (``keypoint_taps``); ``frame`` a 3 x 3 sequence (default ``keypoint_frame("y_up")``); ``joint_map`` /
    ``parents`` sequences of J ints; ``env_mask`` (N,) bool / uint8: envs at 0 are left untouched.  ``raw`` (N, J, 3): the reordered input."""
    a = _lib.KeypointPushArgs()
    a.j3d = _p(j3d, "j3d", torch.float32)
    j = len(parents)
    if j3d.dim() != 3 or tuple(j3d.shape[1:]) != (j, 3):
        raise ValueError(f"j3d: expected (N, {j}, 3), got {tuple(j3d.shape)}")
    n = j3d.shape[0]
    if not 6 <= j <= KEYPOINT_MAX_BODIES:
        raise ValueError(f"keypoint_push: num_bodies {j} not in [6, {KEYPOINT_MAX_BODIES}] (one lane of a half-wave per body and one for the root)")
    if len(joint_map) != j:
        raise ValueError(f"joint_map: {j} entries expected, one per body")
    a.root_ring = _p(root_ring, "root_ring", torch.float32)
    if root_ring.dim() != 3 or root_ring.shape[0] != n or root_ring.shape[2] != 3:
        raise ValueError(f"root_ring: expected ({n}, H, 3), got {tuple(root_ring.shape)}")
    h = root_ring.shape[1]
    if not 1 <= h <= KEYPOINT_MAX_HISTORY:
        raise ValueError(f"keypoint_push: history {h} not in [1, {KEYPOINT_MAX_HISTORY}]")
    a.body_ring, a.prev_pos = _p(body_ring, "body_ring", torch.float32), _p(prev_pos, "prev_pos", torch.float32)
    a.count, a.taps = _p(count, "count", torch.int32), _p(taps, "taps", torch.float32)
    a.pos, a.vel, a.raw = _p(pos, "pos", torch.float32), _p(vel, "vel", torch.float32), _p(raw, "raw", torch.float32)
    for name, t, shape in (("root_ring", root_ring, (n, h, 3)), ("body_ring", body_ring, (n, h, j, 3)), ("count", count, (n,)), ("prev_pos", prev_pos, (n, j, 3)),
                           ("taps", taps, (3, h, h)), ("pos", pos, (n, j, 3)), ("vel", vel, (n, j, 3)), ("raw", raw, (n, j, 3))):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError(f"{name}: expected a contiguous tensor of shape {shape}, got shape {tuple(t.shape)} strides {tuple(t.stride())}")
    if env_mask is not None:
        env_mask = _marshal_mask(env_mask)
        a.env_mask = _p(env_mask, "env_mask", torch.uint8)
        if tuple(env_mask.shape) != (n,):
            raise ValueError(f"env_mask: expected shape ({n},), got {tuple(env_mask.shape)}")
    a.j3d_stride_n, a.j3d_stride_j = j3d.stride(0), j3d.stride(1)
    a.num_envs, a.num_bodies, a.history, a.dt = n, j, h, float(dt)
    a.joint_map[:j] = [int(v) for v in joint_map]
    a.parent_indices[:j] = [int(v) for v in parents]
    if len(mean_limb_lengths) != 5:
        raise ValueError("mean_limb_lengths: five lengths expected (the limbs of bodies 1 .. 5)")
    a.mean_limb_lengths[:] = [float(v) for v in mean_limb_lengths]
    m = keypoint_frame("y_up") if frame is None else frame
    a.frame[:] = [float(m[r][c]) for r in range(3) for c in range(3)]
    _launch("pulse_keypoint_push", ctypes.byref(a))
    return pos, vel


# --------------------------------------------------------------------------- #
# planar ("x3p") fp32-grade GEMM: operands kept pre-split in HBM as three bf16 planes (include/pulse_hip.h section 4b)
# --------------------------------------------------------------------------- #
def planes_pitch(cols):
    """Element pitch of a planes row: the k extent is zero-padded to a multiple of 32 inside the pitch."""
    return (cols + 31) // 32 * 32


def alloc_planes(rows, cols, device):
    """(3, rows, pitch) int16 (bf16 bit patterns), zero-initialised: the pad columns must read as zero."""
    return torch.zeros(3, rows, planes_pitch(cols), dtype=torch.int16, device=device)


def split_planes(x, out=None, *, rows=None, cols=None, transpose=False, row_idx=None, x_off=0, ld_in=None, out_off=0):
    """fp32 matrix -> its three bf16 planes (x == p0 + p1 + p2 exactly).  ``x`` is a 2-D tensor (or a base tensor with x_off / ld_in /
    rows / cols given explicitly); transpose=True writes the planes of x.T."""
    return _to_planes("split_planes", 3, x, out, rows, cols, transpose, row_idx, x_off, ld_in, out_off)


def _to_planes(fn, planes, x, out, rows, cols, transpose, row_idx, x_off, ld_in, out_off):
    """split_planes (``planes`` 3: out (3, rows, pitch)) and to_b16 (``planes`` 1: out (rows, pitch), plane stride 0) on pulse_split_planes."""
    xp = _p(x, "x", off=x_off)
    if ld_in is None:
        if x.dim() != 2 or x.stride(1) != 1:
            raise ValueError(f"{fn}: 2-D tensor with contiguous rows expected (or explicit geometry)")
        ld_in = x.stride(0)
        rows, cols = (x.shape[1], x.shape[0]) if transpose else x.shape
        if row_idx is not None:
            rows = row_idx.numel()
    if out is None:
        out = alloc_planes(rows, cols, x.device) if planes == 3 else alloc_b16(rows, cols, x.device)
    op = _b16(out, f"{fn}: out", out_off)
    if out.dim() != (3 if planes == 3 else 2) or (planes == 3 and out.shape[0] != 3) or out.stride(-1) != 1:
        raise TypeError(f"{fn}: out must be a {'(3, rows, pitch)' if planes == 3 else '(rows, pitch)'} int16 CUDA tensor")
    _launch("pulse_split_planes", xp, ld_in, rows, cols, op, out.stride(0) if planes == 3 else 0, out.stride(-2), 1 if transpose else 0,
            _p(row_idx, "row_idx", _I64))
    return out


def join_planes(p):
    """The fp32 matrix a planes tensor represents (test helper): p0 + p1 + p2 evaluated exactly."""
    f = (p.to(torch.int32) << 16).view(torch.float32)
    return (f[0].double() + f[1].double() + f[2].double()).float()


def alloc_b16(rows, cols, device):
    """(rows, pitch) int16 (bf16 bit patterns), zero-initialised: a single-plane operand / output of gemm_x3p(planes=1)."""
    return torch.zeros(rows, planes_pitch(cols), dtype=torch.int16, device=device)


def to_b16(x, out=None, *, rows=None, cols=None, transpose=False, row_idx=None, x_off=0, ld_in=None, out_off=0):
    """fp32 matrix -> the same matrix rounded to bf16 (round to nearest even), pad columns zero-filled.  Geometry arguments as split_planes."""
    return _to_planes("to_b16", 1, x, out, rows, cols, transpose, row_idx, x_off, ld_in, out_off)


def from_b16(p):
    """The fp32 values of a bf16 bit-pattern tensor."""
    return (p.to(torch.int32) << 16).view(torch.float32)


def make_gemm_x3p_desc(A, B, *, M, N, K, C=None, Cp=None, bias=None, activation=ACT_NONE, epilogue=EPI_BIAS_ACT, aux=None, ldaux=0, C2=None,
                       ldc2=0, ldc=0, batch=1, stride_a=0, stride_b=0, stride_c=0, stride_cp=0, stride_c2=0, stride_bias=0, stride_aux=0,
                       a_off=0, b_off=0, c_off=0, cp_off=0, bias_off=0, aux_off=0, c2_off=0, algo_k=None, algo_n=None, planes=3,
                       a_layout=GEMM_RED_CONTIG, b_layout=GEMM_RED_CONTIG, split_k=1, split_stride=0, lda=None, ldb=None, ldcp=None,
                       out_colsum=None, out_colsum_off=0, stride_out_colsum=0, ld_out_colsum=None, relu_mask8=None, ld_mask8=None, stride_mask8=0,
                       mask8_off=0):
    """planes=3: A / B / Cp are planes tensors (3, rows, pitch) int16.  planes=1 (bf16 operands): (rows, pitch) int16 matrices (or flat
    int16 buffers with lda / ldb / ldcp given), aux may be one too (ReLU-mask / SiLU-derivative epilogues reading bf16 activations).
    *_off are element offsets.  Returns (descriptor, algorithmic FLOPs, tag) like make_gemm_desc."""
    nd = 3 if planes == 3 else 2
    for t, nm, ld in ((A, "A", lda), (B, "B", ldb), (Cp, "Cp", ldcp)):
        if t is None:
            continue
        flat_ok = planes == 1 and ld is not None and t.dim() == 1
        if t.dtype != torch.int16 or not t.is_cuda or not (flat_ok or (t.dim() == nd and t.stride(nd - 1) == 1 and (planes == 1 or t.shape[0] == 3))):
            raise TypeError(f"gemm_x3p: {nm} must be a {'(3, rows, pitch)' if planes == 3 else '(rows, pitch)'} int16 CUDA tensor")
    d = _lib.GemmX3pDesc()
    d.planes = planes
    d.A, d.a_plane_stride, d.lda = _p(A, None, _I16, a_off), (A.stride(0) if planes == 3 else 0), (lda if lda is not None else A.stride(nd - 2))
    d.B, d.b_plane_stride, d.ldb = _p(B, None, _I16, b_off), (B.stride(0) if planes == 3 else 0), (ldb if ldb is not None else B.stride(nd - 2))
    d.a_layout, d.b_layout = a_layout, b_layout
    if C is not None:
        d.C, d.ldc = _p(C, "C", off=c_off), ldc
    if Cp is not None:
        d.Cp, d.c_plane_stride, d.ldcp = _p(Cp, None, _I16, cp_off), (Cp.stride(0) if planes == 3 else 0), (ldcp if ldcp is not None else Cp.stride(nd - 2))
    d.C2, d.ldc2, d.bias = _p(C2, off=c2_off), ldc2, _p(bias, off=bias_off)
    d.aux_is_bf16 = int(aux is not None and aux.dtype == torch.int16)
    d.aux, d.ldaux = _p(aux, None, _I16 if d.aux_is_bf16 else torch.float32, aux_off), ldaux
    d.M, d.N, d.K, d.batch = M, N, K, batch
    d.stride_a, d.stride_b, d.stride_c, d.stride_cp, d.stride_c2 = stride_a, stride_b, stride_c, stride_cp, stride_c2
    d.stride_bias, d.stride_aux = stride_bias, stride_aux
    d.split_k, d.split_stride, d.activation, d.epilogue = split_k, split_stride, activation, epilogue
    if out_colsum is not None:             # (row_tiles(M, N, batch), >= covering columns) fp32: per-row-tile column sums of the stored output
        d.out_colsum, d.stride_out_colsum = _p(out_colsum, "out_colsum", off=out_colsum_off), stride_out_colsum
        d.ld_out_colsum = out_colsum.stride(0) if ld_out_colsum is None else ld_out_colsum
        need = gemm_x3p_row_tiles(M, N, batch)
        if out_colsum.dim() != 2 or out_colsum.shape[0] < need:
            raise ValueError(f"gemm_x3p: out_colsum needs {need} rows (one per row tile)")
    if relu_mask8 is not None:             # uint8 (rows, roundup8(cols) / 8): alloc_relu_mask8; offsets / strides in bytes
        if relu_mask8.dtype != torch.uint8:
            raise TypeError("relu_mask8 must be a uint8 tensor (alloc_relu_mask8)")
        d.relu_mask8 = _p(relu_mask8, None, torch.uint8, int(mask8_off))
        d.ld_mask8, d.stride_mask8 = int(relu_mask8.stride(0) if ld_mask8 is None else ld_mask8), int(stride_mask8)
    flops = 2.0 * M * (algo_n if algo_n else N) * (algo_k if algo_k else K) * batch
    kc_a, kc_b = a_layout == GEMM_RED_CONTIG, b_layout == GEMM_RED_CONTIG
    tag = ("x3p_" if planes == 3 else "b16_") + ("fwd" if kc_a and kc_b else "dx" if kc_a else "dw")
    return d, flops, tag


def gemm_x3p_row_tiles(M, N, batch=1):
    """Row tiles (256 or 128 rows) a pulse_gemm_x3p launch of this shape uses = rows of its out_colsum partials."""
    return int(_lib.load().pulse_gemm_x3p_row_tiles(int(M), int(N), int(batch)))


def gemm_set_option(key, value):
    """Diagnostics knob of the calling host thread (pulse_hip.h, section 4): tests and tools only -- the product path never sets one."""
    _lib.check(_lib.load().pulse_gemm_set_option(int(key), int(value)), "pulse_gemm_set_option")


def launch_gemm_x3p(d, flops=0.0, tag="x3p_fwd", stream=None):
    _launch_desc("pulse_gemm_x3p", d, flops, tag, stream)


def gemm_x3p(A, B, **kw):
    launch_gemm_x3p(*make_gemm_x3p_desc(A, B, **kw))


def linear_forward(x, w, bias=None, activation=ACT_NONE, out=None):
    """Convenience: y = act(x @ w.T + bias) for 2-D row-major tensors with 16-byte aligned rows."""
    _p(x, "x", unit_stride=False), _p(w, "w", unit_stride=False)
    m, k = x.shape
    n = w.shape[0]
    if out is None:
        out = torch.empty(m, n, dtype=torch.float32, device=x.device)
    gemm(x, w, out, M=m, N=n, K=k, lda=x.stride(0), ldb=w.stride(0), ldc=out.stride(0), bias=bias, activation=activation)
    return out


def reduce_slabs(slabs, num_slabs, slab_stride, count, out, scale=1.0, slabs_off=0, out_off=0):
    _launch("pulse_reduce_slabs", _p(slabs, off=slabs_off), num_slabs, slab_stride, count, _p(out, off=out_off), float(scale))


def colsum_partial(x, m, n, ld, num_chunks, partial, ld_partial, x_off=0, partial_off=0):
    _launch("pulse_colsum_partial", _p(x, off=x_off), m, n, ld, num_chunks, _p(partial, off=partial_off), ld_partial)


def rms_copy_supported(x, cols, y, y_cols, raw_out):
    """Can ``rms_normalize(..., raw_out=raw_out)`` run (pulse_rms_normalize_copy's wide-row form)?  Decided by the caller once per buffer set."""
    # the Python mirror of rms_wide_rows(c, 16) in csrc/rms_normalize.hip, plus _copy's own raw_out check: change the two together
    ok = lambda t: t is not None and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0
    c4 = (cols + 3) // 4 * 4
    return bool(ok(x) and ok(y) and ok(raw_out) and 64 <= cols and y_cols <= 3072 and y_cols % 4 == 0 and y_cols >= cols and x.stride(0) >= c4 and
                y.stride(0) >= y_cols and raw_out.stride(0) >= c4 and raw_out.shape[1] >= c4)


def rms_normalize(x, mean, var, *, rows, cols, x_stride, y, y_stride, y_cols=None, row_idx=None, eps=1e-5, clip=5.0,
                  unnorm=False, moment_partials=None, num_blocks=None, planes=None, raw_out=None):
    """``planes``: a (3, rows, pitch) int16 planes tensor that also receives the exact three-way bf16 split of y (layer-1 operand of gemm_x3p).
    ``y`` of dtype int16: the output IS a bf16 matrix (layer-1 operand of the bf16-storage training path); wide rows only.
    ``raw_out``: a (rows, >= cols rounded up to 4) float32 view (any 16-byte aligned row pitch) that also receives the RAW rows read (the rollout's
    record of the observation, see rms_copy_supported); normalising direction, fp32 output, no planes."""
    if num_blocks is None:
        num_blocks = max(1, min(512, rows // 16)) if moment_partials is None else moment_partials.shape[0]
    # the four entries share their leading arguments (the plain one takes the direction before y) and their tail up to num_blocks
    head = (_p(x), x_stride, _p(row_idx), rows, cols, _p(mean), _p(var), eps, clip)
    tail = (_p(y), y_stride, cols if y_cols is None else y_cols, _p(moment_partials), num_blocks)
    if raw_out is not None:
        if unnorm or planes is not None or y.dtype != torch.float32:
            raise ValueError("rms_normalize: raw_out goes with the plain normalising direction only")
        if not raw_out.is_cuda or raw_out.dtype != torch.float32 or raw_out.dim() != 2 or raw_out.stride(1) != 1 or raw_out.shape[0] < rows:
            raise TypeError("rms_normalize: raw_out must be a (>= rows, cols) float32 CUDA view with unit inner stride")
        _launch("pulse_rms_normalize_copy", *head, *tail, raw_out.data_ptr(), raw_out.stride(0))
    elif y.dtype == torch.int16:
        if unnorm or planes is not None or not y.is_cuda or y.stride(-1) != 1:
            raise ValueError("rms_normalize: a bf16 output goes with the normalising direction, without planes")
        _launch("pulse_rms_normalize_b16", *head, *tail)
    elif planes is not None:
        if unnorm:
            raise ValueError("rms_normalize: planes go with the normalising direction only")
        if planes.dtype != torch.int16 or planes.dim() != 3 or planes.shape[0] != 3 or planes.stride(2) != 1 or planes.shape[1] < rows or not planes.is_cuda:
            raise TypeError("rms_normalize: planes must be a (3, >= rows, pitch) int16 CUDA tensor")
        _launch("pulse_rms_normalize_planes", *head, *tail, planes.data_ptr(), planes.stride(0), planes.stride(1))
    else:
        _launch("pulse_rms_normalize", *head, 1 if unnorm else 0, *tail)


def rms_update(mean, var, count, moment_partials, cols, count_old, batch_count):
    _launch("pulse_rms_update", _p(mean), _p(var), _p(count), _p(moment_partials), moment_partials.shape[0], cols, float(count_old), float(batch_count))


def policy_sample(mu, mu_stride, logstd, noise, noise_stride, rows, num_actions, actions, actions_stride, neglogp,
                  neglogp_stride=1, sigmas=None, sigmas_stride=0, value_raw=None, value_stride=0, value_mean=None,
                  value_var=None, values=None, values_stride=0, mu_off=0, actions_off=0, sigmas_off=0, neglogp_off=0,
                  values_off=0, mus_out=None, mus_out_stride=0, mus_out_off=0):
    f32 = torch.float32
    _launch("pulse_policy_sample", _p(mu, "mu", f32, mu_off), mu_stride, _p(logstd, "logstd"), _p(noise, "noise"), noise_stride,
            _p(value_raw, "value_raw"), value_stride, _p(value_mean, "value_mean", _F64), _p(value_var, "value_var", _F64), rows, num_actions,
            _p(actions, "actions", f32, actions_off), actions_stride, _p(sigmas, "sigmas", f32, sigmas_off), sigmas_stride,
            _p(neglogp, "neglogp", f32, neglogp_off), neglogp_stride, _p(values, "values", f32, values_off), values_stride,
            _p(mus_out, "mus_out", f32, mus_out_off), mus_out_stride)


def ppo_loss(*, mu, mu_stride, value, value_stride, logstd, old_logstd, idx, actions, actions_stride, old_mu, old_mu_stride,
             old_neglogp, advantages, old_values, returns, rows, num_actions, e_clip, critic_coef, bounds_loss_coef, clip_value,
             dmu, dmu_stride, dvalue, dvalue_stride, partials, dmu16=None, dmu16_stride=0, dvalue16=None, dvalue16_stride=0, dmu16_off=0, dvalue16_off=0):
    a = PpoLossArgs()
    a.mu, a.mu_stride, a.value, a.value_stride, a.logstd = _p(mu), mu_stride, _p(value), value_stride, _p(logstd)
    a.idx, a.actions, a.actions_stride = _p(idx), _p(actions), actions_stride
    a.old_mu, a.old_mu_stride, a.old_logstd = _p(old_mu), old_mu_stride, _p(old_logstd)
    a.old_neglogp, a.advantages, a.old_values, a.returns = _p(old_neglogp), _p(advantages), _p(old_values), _p(returns)
    a.rows, a.num_actions = rows, num_actions
    a.e_clip, a.critic_coef = float(e_clip), float(critic_coef)
    a.has_bounds_loss = 0 if bounds_loss_coef is None else 1
    a.bounds_loss_coef = 0.0 if bounds_loss_coef is None else float(bounds_loss_coef)
    a.clip_value = 1 if clip_value else 0
    a.dmu, a.dmu_stride, a.dvalue, a.dvalue_stride = _p(dmu), dmu_stride, _p(dvalue), dvalue_stride
    a.partials, a.num_blocks = _p(partials), partials.shape[0]
    if dmu16 is not None:                  # bf16 copies of the head gradients (int16 bit patterns; *_off in bf16 elements)
        if dvalue16 is None:
            raise TypeError("ppo_loss: dmu16 goes with dvalue16")
        a.dmu16, a.dmu16_stride = _b16(dmu16, "ppo_loss: dmu16", dmu16_off), dmu16_stride
        a.dvalue16, a.dvalue16_stride = _b16(dvalue16, "ppo_loss: dvalue16", dvalue16_off), dvalue16_stride
    _launch("pulse_ppo_loss", ctypes.byref(a))


def advantage_normalize(returns, values, adv_out, partials):
    """adv = (returns - values - mean) / (std + 1e-8) over flat tensors (common_agent.py:589-599)."""
    n = returns.numel()
    _launch("pulse_advantage_moments", _p(returns), _p(values), n, _p(adv_out), _p(partials), partials.shape[0])
    _launch("pulse_advantage_normalize", _p(adv_out), n, _p(partials), partials.shape[0])
    return adv_out


def sqnorm_partial(x, count, partials):
    xp, pp = _p(x, "x"), _p(partials, "partials")
    if x.numel() < count or not x.is_contiguous():
        raise ValueError(f"sqnorm_partial: x must be a contiguous buffer of at least {count} floats")
    _launch("pulse_sqnorm_partial", xp, count, pp, partials.numel())


def disc_head(logits, b, scale, dlogits, stats):
    """AMPAgent._disc_loss head on the (3b, 1) logit column (any row stride): fills ``dlogits`` (same shape) and ``stats`` (8 floats:
    pred loss, agent BCE, demo BCE, agent acc, demo acc, agent logit mean, demo logit mean, 0)."""
    lp, dp, sp = _p(logits, "logits"), _p(dlogits, "dlogits"), _p(stats, "stats")
    if logits.shape[0] != 3 * b or dlogits.shape[0] != 3 * b or stats.numel() < 8 or not stats.is_contiguous():
        raise ValueError("disc_head: logits / dlogits must have 3b rows and stats 8 contiguous floats")
    _launch("pulse_disc_head", lp, logits.stride(0), b, float(scale), dp, dlogits.stride(0), sp)


def disc_head_b16(logits, b, scale, dlogits16, stats, dlogits=None, bias_grad=None):
    """disc_head writing the logit gradients as bf16 (dlogits16: int16 (>= 3b, pitch) tensor, column 0) and optionally as fp32 too;
    ``bias_grad`` (a float32 view, element 0): receives their sum = the logit bias' gradient."""
    lp, sp, dp, bp = _p(logits, "logits"), _p(stats, "stats"), _p(dlogits, "dlogits"), _p(bias_grad, "bias_grad", unit_stride=False)
    if dlogits16.dtype != torch.int16 or not dlogits16.is_cuda or dlogits16.shape[0] < 3 * b or logits.shape[0] != 3 * b or stats.numel() < 8:
        raise ValueError("disc_head_b16: logits must have 3b rows, dlogits16 be an int16 CUDA tensor of >= 3b rows, stats 8 floats")
    _launch("pulse_disc_head_b16", lp, logits.stride(0), b, float(scale), dp, dlogits.stride(0) if dlogits is not None else 0, dlogits16.data_ptr(),
            dlogits16.stride(0), sp, bp)


def transpose_to_b16(x, out, *, rows, cols, ld_in, ld_out, batch=1, stride_in=0, stride_out=0, x_off=0, out_off=0):
    """out[z][c][r] = bf16(x[z][r][c]); x fp32 base tensor (+ x_off floats), out int16 base tensor (+ out_off elements)."""
    _launch("pulse_transpose_to_b16", _p(x, "x", off=x_off), ld_in, rows, cols, _b16(out, "transpose_to_b16: out", out_off), ld_out, batch, stride_in,
            stride_out)


def colsum_partial_b16(x, m, n, ld, num_chunks, partial, ld_partial, x_off=0, partial_off=0):
    _launch("pulse_colsum_partial_b16", _b16(x, "colsum_partial_b16: x", x_off), m, n, ld, num_chunks, _p(partial, "partial", off=partial_off), ld_partial)


def disc_penalty(G, rows, cols, scale, partials, out32=None, out16=None, out32_off=0, out16_off=0, ld32=0, ld16=0):
    """partials[block] = sum G^2; out32 / out16 (+ element offsets) = scale * G as fp32 / bf16."""
    _launch("pulse_disc_penalty", _p(G, "G"), G.stride(0), rows, cols, float(scale), _p(out32, "out32", off=out32_off), ld32,
            _b16(out16, "disc_penalty: out16", out16_off) if out16 is not None else None, ld16, _p(partials, "partials"), partials.numel())


def disc_reg(flat, grad, ranges, partials):
    """ranges: [(offset, length, alpha)] (<= 4).  grad[off + i] += alpha * flat[off + i]; partials (blocks, 4) = per-block sums of flat[range]^2."""
    fp, gp, pp = _p(flat, "flat"), _p(grad, "grad"), _p(partials, "partials")
    n = len(ranges)
    if not 1 <= n <= 4 or partials.dim() != 2 or partials.shape[1] != 4 or not partials.is_contiguous():
        raise ValueError("disc_reg: 1..4 ranges, partials (blocks, 4) contiguous")
    offs = (ctypes.c_int64 * n)(*[int(r[0]) for r in ranges])
    lens = (ctypes.c_int64 * n)(*[int(r[1]) for r in ranges])
    als = (ctypes.c_float * n)(*[float(r[2]) for r in ranges])
    _launch("pulse_disc_reg", fp, gp, n, offs, lens, als, pp, partials.shape[0])


def carve_reduce_regions(base, parts, max_regions=8):
    """Regions of a fused gradient reduce (ReduceGrads).  ``base``: [(offset, count, nslabs)], the slab-summed ranges of the flat gradient in
    order; ``parts``: [(dst_offset, count, rows, src)], ranges whose value is the ordered sum of ``rows`` partial rows of the 2-D tensor ``src``
    (Plan.partial_reduces).  Every part is carved out of the base range that contains it and becomes a region with its own source.
    -> (regions, fused): fused is False -- and the regions are the plain base ranges -- when there is no part, a part straddles base ranges or
    overlaps another, an offset / count / row stride is not a multiple of 4 floats, or more than ``max_regions`` regions would result; the
    caller then keeps the plan's small reduce launches."""
    plain = [(o, c, n, 0.0) for o, c, n in base]
    todo = sorted(parts, key=lambda r: r[0])
    if not todo:
        return plain, False
    regions, used = [], 0
    for off, cnt, ns in base:
        pos, end = off, off + cnt
        for doff, dcnt, rows, src in todo:
            if doff < off or doff >= end:
                continue
            if doff < pos or doff + dcnt > end or doff % 4 or dcnt % 4 or src.stride(0) % 4 or rows < 1:
                return plain, False
            if doff > pos:
                regions.append((pos, doff - pos, ns, 0.0))
            regions.append((doff, dcnt, rows, 0.0, src, src.stride(0)))
            pos = doff + dcnt
            used += 1
        if end > pos:
            regions.append((pos, end - pos, ns, 0.0))
    if used != len(todo) or len(regions) > max_regions:
        return plain, False
    return regions, True


class ReduceGrads:
    """A pre-built pulse_reduce_grads launch: regions = [(offset, count, nslabs, alpha[, src, src_stride])] of a flat gradient buffer; a region
    with ``src`` (a float32 device tensor) sums nslabs rows of that buffer (row stride ``src_stride`` floats) instead of the slabs."""

    def __init__(self, slabs, slab_stride, regions, out, flat=None):
        n = len(regions)
        if not 1 <= n <= 32:
            raise ValueError("ReduceGrads: 1..32 regions")
        _p(slabs, "slabs"), _p(out, "out"), _p(flat, "flat")
        self.n = n
        self.offs = (ctypes.c_int64 * n)(*[int(r[0]) for r in regions])
        self.cnts = (ctypes.c_int64 * n)(*[int(r[1]) for r in regions])
        self.nsl = (ctypes.c_int32 * n)(*[int(r[2]) for r in regions])
        self.als = (ctypes.c_float * n)(*[float(r[3]) for r in regions])
        self._src_keep = [r[4] if len(r) > 4 else None for r in regions]          # (the tensors stay alive with the launch)
        for t in self._src_keep:
            _p(t, "region src", unit_stride=False)
        self.srcs = (ctypes.c_void_p * n)(*[(t.data_ptr() if t is not None else None) for t in self._src_keep])
        self.sstr = (ctypes.c_int64 * n)(*[(int(r[5]) if len(r) > 5 and r[4] is not None else 0) for r in regions])
        self.slabs, self.stride, self.out, self.flat = slabs, int(slab_stride), out, flat
        self.has_alpha = any(float(r[3]) != 0.0 for r in regions)

    def run(self, scale=1.0, sq_partials=None, w2_partials=None, num_blocks=1024, alphas=None):
        sq, w2 = _p(sq_partials, "sq_partials"), _p(w2_partials, "w2_partials")
        if alphas is not None:                       # per-call regulariser coefficients (one per region)
            if len(alphas) != self.n:
                raise ValueError("ReduceGrads: one alpha per region")
            self.als = (ctypes.c_float * self.n)(*[float(a) for a in alphas])
            self.has_alpha = any(float(a) != 0.0 for a in alphas)
        if sq_partials is not None:
            num_blocks = sq_partials.numel()
        if w2_partials is not None and (w2_partials.numel() != 8 * num_blocks or not w2_partials.is_contiguous()):
            raise ValueError("ReduceGrads: w2_partials must be (num_blocks, 8) contiguous, num_blocks = sq_partials.numel() (default 1024)")
        if (w2_partials is not None or self.has_alpha) and self.flat is None:
            raise ValueError("ReduceGrads: regulariser terms need the flat parameter buffer")
        _launch("pulse_reduce_grads", self.slabs.data_ptr(), self.stride, self.n, self.offs, self.cnts, self.nsl, self.als, self.srcs, self.sstr,
                self.out.data_ptr(), float(scale), _p(self.flat), sq, w2, num_blocks)


def disc_reward(logits, n, scale, out):
    _launch("pulse_disc_reward", _p(logits, "logits", unit_stride=False), logits.stride(0), n, float(scale), _p(out, "out", unit_stride=False), out.stride(0))


def adam_step(params, grads, exp_avg, exp_avg_sq, count, *, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
              max_norm=0.0, sqnorm_partials=None, grad_norm_out=None):
    for t, nm in ((params, "params"), (grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"), (sqnorm_partials, "sqnorm_partials"),
                  (grad_norm_out, "grad_norm_out")):
        _p(t, nm)
        if t is not None and nm in ("params", "grads", "exp_avg", "exp_avg_sq") and (t.numel() < count or not t.is_contiguous()):
            raise ValueError(f"adam_step: {nm} must be a contiguous buffer of at least {count} floats")
    _launch("pulse_adam_step", _p(params), _p(grads), _p(exp_avg), _p(exp_avg_sq), count, float(lr), beta1, beta2, eps, weight_decay, int(step),
            float(max_norm), _p(sqnorm_partials), sqnorm_partials.numel() if sqnorm_partials is not None else 0, _p(grad_norm_out))


def adam_step_multi(groups, *, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=0.0, sqnorm_partials=None, grad_norm_out=None):
    """adam_step over several flat buffers -- groups = [(params, grads, exp_avg, exp_avg_sq, count)] -- in ONE launch (pulse_adam_step_multi)."""
    n = len(groups)
    if not 1 <= n <= 4:
        raise ValueError("adam_step_multi: 1..4 groups")
    sq, gn = _p(sqnorm_partials, "sqnorm_partials"), _p(grad_norm_out, "grad_norm_out")
    cols = [[], [], [], []]
    for g in groups:
        for k, nm in enumerate(("params", "grads", "exp_avg", "exp_avg_sq")):
            cols[k].append(_p(g[k], nm))
            if g[k].numel() < g[4] or not g[k].is_contiguous():
                raise ValueError(f"adam_step_multi: {nm} must be a contiguous buffer of at least {g[4]} floats")
    arrs = [(ctypes.c_void_p * n)(*c) for c in cols]
    counts = (ctypes.c_int64 * n)(*[int(g[4]) for g in groups])
    _launch("pulse_adam_step_multi", n, *arrs, counts, float(lr), beta1, beta2, eps, weight_decay, int(step), float(max_norm), sq,
            sqnorm_partials.numel() if sqnorm_partials is not None else 0, gn)


def rollout_record(*, rewards, dones, terminate, value_raw, value_stride, value_mean, value_var, value_eps, buf_rewards, buf_next_values,
                   buf_dones, env_stride, current_rewards, current_lengths, meter_rewards, meter_lengths, meter_max_size, done_mask,
                   reward_scale=1.0, reward_shift=0.0, buf_terminate=None, meter_partials=None):
    """play_steps bookkeeping of one rollout step in one launch (include/pulse_hip.h section 2c)."""
    a = _lib.RolloutRecordArgs()
    a.num_envs = rewards.numel()
    a.rewards, a.reward_scale, a.reward_shift = _p(rewards, "rewards"), float(reward_scale), float(reward_shift)
    a.dones, a.terminate = _p(dones, "dones", _I64), _p(terminate, "terminate", _I64)
    a.value_raw, a.value_stride = _p(value_raw), int(value_stride)
    a.value_mean, a.value_var, a.value_eps = _p(value_mean, "value_mean", _F64), _p(value_var, "value_var", _F64), float(value_eps)
    a.buf_rewards, a.buf_next_values, a.buf_dones, a.env_stride = _p(buf_rewards), _p(buf_next_values), _p(buf_dones), int(env_stride)
    a.current_rewards, a.current_lengths = _p(current_rewards, "current_rewards"), _p(current_lengths, "current_lengths")
    a.meter_rewards, a.meter_lengths, a.meter_max_size = _p(meter_rewards, "meter_rewards"), _p(meter_lengths, "meter_lengths"), float(meter_max_size)
    a.done_mask, a.buf_terminate = _p(done_mask, "done_mask", torch.uint8), _p(buf_terminate)
    if meter_partials is not None:          # (blocks, 4) row of this step: the meter updates are applied later by rollout_meters
        a.meter_partials, a.meter_blocks = _p(meter_partials, "meter_partials"), meter_partials.shape[0]
        if meter_partials.dim() != 2 or meter_partials.shape[1] != 4 or not meter_partials.is_contiguous():
            raise ValueError("rollout_record: meter_partials must be a contiguous (blocks, 4) tensor")
    _launch("pulse_rollout_record", ctypes.byref(a))


def rollout_meters(partials, meter_rewards, meter_lengths, meter_max_size):
    """The deferred AverageMeter updates of a rollout: partials (steps, blocks, 4) from rollout_record(meter_partials=partials[step])."""
    pp, rp, lp = _p(partials, "partials"), _p(meter_rewards, "meter_rewards"), _p(meter_lengths, "meter_lengths")
    if partials.dim() != 3 or partials.shape[2] != 4 or not partials.is_contiguous():
        raise ValueError("rollout_meters: partials must be a contiguous (steps, blocks, 4) tensor")
    _launch("pulse_rollout_meters", pp, partials.shape[0], partials.shape[1], rp, lp, float(meter_max_size))


def kinematic_sim_step(target_rb, noise_rb, rb, target_dof_pos, noise_dof_pos, dof_pos, target_dof_vel, noise_dof_vel, dof_vel, force_src,
                       dof_force):
    n, j = rb.shape[0], rb.shape[1]
    _launch("pulse_kinematic_sim_step", _p(target_rb), _p(noise_rb), _p(rb), n, j, _p(target_dof_pos), _p(noise_dof_pos), _p(dof_pos), _p(target_dof_vel),
            _p(noise_dof_vel), _p(dof_vel), _p(force_src), _p(dof_force), dof_pos.shape[1])

