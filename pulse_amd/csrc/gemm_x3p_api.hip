// pulse_gemm_x3p: argument checks, tile choice and dispatch to the planar kernels (gemm_x3p.hip: three planes, and one plane on 128-row tiles;
// gemm_b16.hip: one plane on 256-row tiles), and pulse_split_planes, which writes the planes of a matrix that no kernel's epilogue produced.
#include "gemm_planar.h"

namespace pulse {

// ---- fp32 matrix -> three bf16 planes (optionally transposed); pad columns [cols, ld_out) of every written row are zero-filled ----
// out plane p, element (r, c) at out[p * plane_stride + r * ld_out + c].  transpose: out(r, c) = in(c, r) (rows_out = cols_in).
__global__ void __launch_bounds__(256) split_planes_kernel(const float* __restrict__ in, long long ld_in, int rows_out, int cols_out,
                                                          unsigned short* __restrict__ out, long long plane_stride, int ld_out, int transpose,
                                                          const long long* __restrict__ row_idx, int vec_in) {
    const int pieces = ld_out >> 3;                                 // 16-byte pieces per output row
    const long long total = (long long)rows_out * pieces;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / pieces), c0 = (int)(i - (long long)r * pieces) * 8;
        float v[8];
        if (!transpose) {
            const float* src = in + (row_idx ? row_idx[r] : (long long)r) * ld_in + c0;
            if (vec_in && c0 + 7 < cols_out) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
                v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = c0 + k < cols_out ? src[k] : 0.f;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = c0 + k < cols_out ? in[(long long)(c0 + k) * ld_in + r] : 0.f;
        }
        u32x4 q0, q1, q2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned x0, x1, x2;
            split_pair3(v[2 * k], v[2 * k + 1], x0, x1, x2);
            q0[k] = x0; q1[k] = x1; q2[k] = x2;
        }
        unsigned short* o = out + (long long)r * ld_out + c0;
        *reinterpret_cast<u32x4*>(o) = q0;
        if (plane_stride) {                                         // plane_stride 0: a plain bf16 matrix (plane 0 only)
            *reinterpret_cast<u32x4*>(o + plane_stride) = q1;
            *reinterpret_cast<u32x4*>(o + 2 * plane_stride) = q2;
        }
    }
}

}  // namespace pulse

using namespace pulse;

extern "C" {

int pulse_sizeof_gemm_x3p_desc(void) { return (int)sizeof(pulse_gemm_x3p_desc); }

int pulse_split_planes(const float* in, int64_t ld_in, int32_t rows_out, int32_t cols_out, void* out, int64_t plane_stride, int32_t ld_out,
                       int32_t transpose, const int64_t* row_idx, pulse_stream_t s) {
    PULSE_REQUIRE(rows_out >= 0 && cols_out >= 0, "pulse_split_planes: negative size");
    if (rows_out == 0) return PULSE_OK;
    PULSE_REQUIRE(in && out, "pulse_split_planes: null pointer");
    PULSE_REQUIRE(ld_out % 8 == 0 && ld_out >= cols_out && (plane_stride == 0 || plane_stride >= (int64_t)rows_out * ld_out) && plane_stride % 8 == 0,
                  "pulse_split_planes: ld_out must be a multiple of 8 covering cols_out, plane_stride a multiple of 8 covering the plane (or 0: one plane)");
    PULSE_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "pulse_split_planes: out must be 16-byte aligned");
    const int vec_in = !transpose && (ld_in % 4) == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;      // 16-byte loads when the rows allow them
    PULSE_REQUIRE(!(transpose && row_idx), "pulse_split_planes: row_idx with transpose is not supported");
    const long long total = (long long)rows_out * (ld_out / 8);
    long long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(s), in, (long long)ld_in, rows_out, cols_out,
                       reinterpret_cast<unsigned short*>(out), (long long)plane_stride, ld_out, transpose, reinterpret_cast<const long long*>(row_idx), vec_in);
    return check_launch("pulse_split_planes");
}

static bool xp_big_tiles(int M, int N, int batch, int split_k) {
    // 256-row tiles when they still give every CU a workgroup; otherwise 128-row tiles (4 waves)
    const long long t256 = (long long)((M + 255) / 256) * ((N + PBN - 1) / PBN) * batch * split_k;
    return t256 >= 256 || M > 128 * 64;
}

// 256 x 256 tiles (gemm_b16w_kernel) when they do not cost the launch a round of workgroups: a wide workgroup does the work of two narrow
// ones, so it wins whenever 2 x rounds(wide) <= rounds(narrow) on the 256 CUs.  gemm option 3: 1 = never, 2 = whenever the tile has a second half.
static bool xp_wide_tiles(int M, int N, int batch, int split_k) {
    const int opt = gemm_option(3);
    if (opt == 1 || N <= PBN) return false;
    if (opt == 2) return true;
    const long long tm = (M + 255) / 256, bs = (long long)batch * split_k;
    const long long tn = tm * ((N + PBN - 1) / PBN) * bs, tw = tm * ((N + 255) / 256) * bs;
    return 2 * ((tw + 255) / 256) <= (tn + 255) / 256;
}

int pulse_gemm_x3p_row_tiles(int32_t M, int32_t N, int32_t batch) {
    if (M <= 0 || N <= 0 || batch <= 0) return 0;
    return xp_big_tiles(M, N, batch, 1) ? (M + 255) / 256 : (M + 127) / 128;
}

int pulse_gemm_x3p(const pulse_gemm_x3p_desc* d, pulse_stream_t s) {
    PULSE_REQUIRE(d != nullptr, "pulse_gemm_x3p: null descriptor");
    PULSE_REQUIRE(d->M >= 0 && d->N >= 0 && d->K >= 0, "pulse_gemm_x3p: negative size");
    if (d->M == 0 || d->N == 0 || d->batch == 0) return PULSE_OK;
    PULSE_REQUIRE(d->A && d->B && (d->C || d->Cp), "pulse_gemm_x3p: null operand / no output");
    PULSE_REQUIRE(d->batch >= 1 && d->split_k >= 1, "pulse_gemm_x3p: batch / split_k must be >= 1");
    PULSE_REQUIRE(d->planes == 0 || d->planes == 1 || d->planes == 3, "pulse_gemm_x3p: planes must be 3 (fp32-grade; 0 means 3) or 1 (bf16 operands)");
    const int npl = d->planes == 1 ? 1 : 3;
    const bool akc = d->a_layout == PULSE_GEMM_RED_CONTIG, bkc = d->b_layout == PULSE_GEMM_RED_CONTIG;
    PULSE_REQUIRE(akc == bkc || (akc && !bkc), "pulse_gemm_x3p: layout combination (A out-contiguous, B reduction-contiguous) unsupported");
    PULSE_REQUIRE((d->lda % 8) == 0 && (d->ldb % 8) == 0 && (d->a_plane_stride % 8) == 0 && (d->b_plane_stride % 8) == 0 &&
                  (d->stride_a % 8) == 0 && (d->stride_b % 8) == 0, "pulse_gemm_x3p: operand pitches / strides must be multiples of 8 elements");
    PULSE_REQUIRE((reinterpret_cast<uintptr_t>(d->A) & 15) == 0 && (reinterpret_cast<uintptr_t>(d->B) & 15) == 0, "pulse_gemm_x3p: A / B must be 16-byte aligned");
    const int kpad = (d->K + PK - 1) / PK * PK;
    // reduction-contiguous rows must hold the zero-padded k extent; [k][out] operands must hold roundup8(extent) columns
    PULSE_REQUIRE(akc ? d->lda >= kpad : d->lda >= ((d->M + 7) & ~7), "pulse_gemm_x3p: lda too small (k is padded to a multiple of 32 with zeros)");
    PULSE_REQUIRE(bkc ? d->ldb >= kpad : d->ldb >= ((d->N + 7) & ~7), "pulse_gemm_x3p: ldb too small (k is padded to a multiple of 32 with zeros)");
    PULSE_REQUIRE(d->split_k == 1 || (akc == false), "pulse_gemm_x3p: split-K is for the [red][out] x [red][out] (weight-gradient) form");
    PULSE_REQUIRE(!d->C || d->ldc >= d->N, "pulse_gemm_x3p: ldc too small");
    PULSE_REQUIRE(!d->C || ((reinterpret_cast<uintptr_t>(d->C) & 15) == 0 && (d->ldc % 4) == 0 && (d->stride_c % 4) == 0 && (d->split_stride % 4) == 0),
                  "pulse_gemm_x3p: C rows must be 16-byte aligned");
    PULSE_REQUIRE(!d->Cp || ((reinterpret_cast<uintptr_t>(d->Cp) & 15) == 0 && (d->ldcp % 8) == 0 && d->ldcp >= ((d->N + 7) & ~7) && (d->c_plane_stride % 8) == 0 &&
                             (d->stride_cp % 8) == 0), "pulse_gemm_x3p: Cp rows must be 16-byte aligned and hold roundup8(N) columns");
    PULSE_REQUIRE(!d->Cp || d->split_k == 1, "pulse_gemm_x3p: split-K slabs carry no planes");
    PULSE_REQUIRE(d->epilogue >= 0 && d->epilogue <= 2 && d->activation >= 0 && d->activation <= 2, "pulse_gemm_x3p: bad epilogue / activation");
    PULSE_REQUIRE(d->epilogue == 0 || d->aux != nullptr || (d->epilogue == PULSE_EPI_RELU_GRAD && d->relu_mask8 != nullptr),
                  "pulse_gemm_x3p: gradient epilogue needs aux (or, for relu-grad, relu_mask8)");
    const bool mask8_on = d->relu_mask8 != nullptr && ((d->epilogue == PULSE_EPI_RELU_GRAD && d->aux == nullptr) ||
                                                       (d->epilogue == PULSE_EPI_BIAS_ACT && d->activation == PULSE_ACT_RELU));
    PULSE_REQUIRE(!mask8_on || (d->ld_mask8 >= (d->N + 7) / 8 && d->split_k == 1), "pulse_gemm_x3p: relu_mask8 needs ld_mask8 >= roundup8(N) / 8 and no split-K");
    if (d->aux_is_bf16) {
        PULSE_REQUIRE(!d->aux || ((reinterpret_cast<uintptr_t>(d->aux) & 15) == 0 && (d->ldaux % 8) == 0 && (d->stride_aux % 8) == 0 && d->ldaux >= ((d->N + 7) & ~7)),
                      "pulse_gemm_x3p: bf16 aux rows must be 16-byte aligned and hold roundup8(N) columns");
    } else {
        PULSE_REQUIRE(!d->aux || ((reinterpret_cast<uintptr_t>(d->aux) & 15) == 0 && (d->ldaux % 4) == 0 && (d->stride_aux % 4) == 0), "pulse_gemm_x3p: aux rows must be 16-byte aligned");
    }
    PULSE_REQUIRE(!d->C2 || ((reinterpret_cast<uintptr_t>(d->C2) & 15) == 0 && (d->ldc2 % 4) == 0 && (d->stride_c2 % 4) == 0), "pulse_gemm_x3p: C2 rows must be 16-byte aligned");
    PULSE_REQUIRE(d->split_k == 1 || (d->epilogue == 0 && d->activation == 0 && d->bias == nullptr), "pulse_gemm_x3p: split-K slabs carry no epilogue");
    PULSE_REQUIRE(d->rowsum == nullptr, "pulse_gemm_x3p: rowsum is not implemented in this build");
    PULSE_REQUIRE(!d->out_colsum || (d->split_k == 1 && d->ld_out_colsum >= d->N), "pulse_gemm_x3p: out_colsum needs split_k == 1 and a pitch covering N");

    XpArgs g;
    g.A = reinterpret_cast<const unsigned short*>(d->A); g.B = reinterpret_cast<const unsigned short*>(d->B);
    g.pa = d->a_plane_stride; g.pb = d->b_plane_stride; g.lda = d->lda; g.ldb = d->ldb;
    g.C = d->C; g.C2 = d->C2; g.Cp = reinterpret_cast<unsigned short*>(d->Cp); g.bias = d->bias;
    g.aux = d->aux_is_bf16 ? nullptr : d->aux;
    g.aux16 = d->aux_is_bf16 ? reinterpret_cast<const unsigned short*>(d->aux) : nullptr;
    g.pc = d->c_plane_stride; g.ldc = d->ldc; g.ldc2 = d->ldc2; g.ldcp = d->ldcp; g.ldaux = d->ldaux;
    g.M = d->M; g.N = d->N; g.K = d->K;
    g.sA = d->stride_a; g.sB = d->stride_b; g.sC = d->stride_c; g.sC2 = d->stride_c2; g.sCp = d->stride_cp; g.sBias = d->stride_bias; g.sAux = d->stride_aux;
    g.batch = d->batch; g.splitk = d->split_k;
    const bool big = xp_big_tiles(d->M, d->N, d->batch, d->split_k);
    const bool ring = npl == 1 && big;                               // bf16 storage, 256-row tiles: the three-stage ring kernel
    const bool wide = ring && xp_wide_tiles(d->M, d->N, d->batch, d->split_k);     // ... or its 256 x 256 form
    const int kq = ring ? 2 * PK : npl == 1 ? 3 * PK : PK;           // split-K chunks are whole pipeline stages
    int kchunk = (d->K + d->split_k - 1) / d->split_k;
    kchunk = ((kchunk + kq - 1) / kq) * kq;
    g.kchunk = kchunk > 0 ? kchunk : kq;
    g.sSplit = d->split_stride;
    g.act = d->activation; g.epi = d->epilogue;
    g.rowsum = d->rowsum; g.sRowsum = d->stride_rowsum;
    g.colsum = d->out_colsum; g.sColsum = d->stride_out_colsum; g.ldcs = d->ld_out_colsum;
    g.mask8 = mask8_on ? d->relu_mask8 : nullptr; g.ldm8 = d->ld_mask8; g.sM8 = d->stride_mask8;
    g.general_rows = gemm_option(9);
    g.dbg = gemm_debug_buffer();
    g.tiles_m = big ? (d->M + 255) / 256 : (d->M + 127) / 128;
    g.tiles_n = wide ? (d->N + 2 * PBN - 1) / (2 * PBN) : (d->N + PBN - 1) / PBN;
    PULSE_REQUIRE((long long)d->lda * 300 < (1LL << 29) && (long long)d->ldb * 300 < (1LL << 29), "pulse_gemm_x3p: pitch too large for 32-bit tile-relative offsets");
    // [red][out] operands advance lda elements per k row: the whole k extent of a split must stay inside the 32-bit scalar offset
    PULSE_REQUIRE(akc || (long long)g.kchunk * d->lda * 2 < (1LL << 31), "pulse_gemm_x3p: split the reduction further (k extent x pitch exceeds 2 GiB)");
    PULSE_REQUIRE(bkc || (long long)g.kchunk * d->ldb * 2 < (1LL << 31), "pulse_gemm_x3p: split the reduction further (k extent x pitch exceeds 2 GiB)");
    const hipStream_t st = as_stream(s);
    if (wide) return launch_gemm_b16w(g, akc, bkc, st);
    if (ring) return launch_gemm_b16r(g, akc, bkc, st);
    return launch_gemm_x3p(g, akc, bkc, npl, big, st);              // three planes, or one on 128-row tiles
}
}
