// pulse_gemm_f32: the entry point of the fp32-storage GEMMs.  Validates the descriptor, fills the kernels' argument block and chooses the kernel
// family and tiling (fp32 MFMA / bf16 MFMA: gemm_f32.hip; x3 128 x 128 or 64 x 128: gemm_x3.hip; x3 256 x 256: gemm_x3w.hip; x3 skinny-N:
// gemm_x3s.hip).  Also here: the calling thread's diagnostic state and the two small reductions that finish a split-K / bias-gradient launch.
#include <cstdlib>
#include "common.h"
#include "gemm_shared.h"

namespace pulse {

// ---- deterministic reduction of split-K slabs (and of column-sum partials) ---------------------
__global__ void __launch_bounds__(256) reduce_slabs_kernel(const float* __restrict__ slabs, int nslab, long long slab_stride,
                                                          long long count, float* __restrict__ out, float scale) {
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < count; i += (long long)gridDim.x * blockDim.x * 4) {
        if (i + 3 < count) {
            // four independent chains (slabs k, k+1, k+2, k+3 of every group of four), combined in a fixed order: the loads of a group are in
            // flight together (a 64-row reduce of a few KB was one dependent L2 round trip per row: 16 us)
            float4 s = *reinterpret_cast<const float4*>(slabs + i);
            float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1, s3 = s1;
            int k = 1;
            for (; k + 15 < nslab; k += 16) {                  // [r6] sixteen slabs in flight, added in the same order (reduce_grads_kernel, b16_ops.hip)
                float4 v[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) v[u] = *reinterpret_cast<const float4*>(slabs + (k + u) * slab_stride + i);
#pragma unroll
                for (int u = 0; u < 16; u += 4) {
                    s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w;
                    s1.x += v[u + 1].x; s1.y += v[u + 1].y; s1.z += v[u + 1].z; s1.w += v[u + 1].w;
                    s2.x += v[u + 2].x; s2.y += v[u + 2].y; s2.z += v[u + 2].z; s2.w += v[u + 2].w;
                    s3.x += v[u + 3].x; s3.y += v[u + 3].y; s3.z += v[u + 3].z; s3.w += v[u + 3].w;
                }
            }
            for (; k + 3 < nslab; k += 4) {
                const float4 v0 = *reinterpret_cast<const float4*>(slabs + k * slab_stride + i);
                const float4 v1 = *reinterpret_cast<const float4*>(slabs + (k + 1) * slab_stride + i);
                const float4 v2 = *reinterpret_cast<const float4*>(slabs + (k + 2) * slab_stride + i);
                const float4 v3 = *reinterpret_cast<const float4*>(slabs + (k + 3) * slab_stride + i);
                s.x += v0.x; s.y += v0.y; s.z += v0.z; s.w += v0.w;
                s1.x += v1.x; s1.y += v1.y; s1.z += v1.z; s1.w += v1.w;
                s2.x += v2.x; s2.y += v2.y; s2.z += v2.z; s2.w += v2.w;
                s3.x += v3.x; s3.y += v3.y; s3.z += v3.z; s3.w += v3.w;
            }
            const int rem = nslab - k;                          // the last one to three slabs onto chain 0 in order, loads issued together
            if (rem == 3) {
                const float4 t0 = *reinterpret_cast<const float4*>(slabs + k * slab_stride + i);
                const float4 t1 = *reinterpret_cast<const float4*>(slabs + (k + 1) * slab_stride + i);
                const float4 t2 = *reinterpret_cast<const float4*>(slabs + (k + 2) * slab_stride + i);
                s.x += t0.x; s.y += t0.y; s.z += t0.z; s.w += t0.w;
                s.x += t1.x; s.y += t1.y; s.z += t1.z; s.w += t1.w;
                s.x += t2.x; s.y += t2.y; s.z += t2.z; s.w += t2.w;
            } else if (rem == 2) {
                const float4 t0 = *reinterpret_cast<const float4*>(slabs + k * slab_stride + i);
                const float4 t1 = *reinterpret_cast<const float4*>(slabs + (k + 1) * slab_stride + i);
                s.x += t0.x; s.y += t0.y; s.z += t0.z; s.w += t0.w;
                s.x += t1.x; s.y += t1.y; s.z += t1.z; s.w += t1.w;
            } else if (rem == 1) {
                const float4 t0 = *reinterpret_cast<const float4*>(slabs + k * slab_stride + i);
                s.x += t0.x; s.y += t0.y; s.z += t0.z; s.w += t0.w;
            }
            s.x = (s.x + s1.x) + (s2.x + s3.x); s.y = (s.y + s1.y) + (s2.y + s3.y); s.z = (s.z + s1.z) + (s2.z + s3.z); s.w = (s.w + s1.w) + (s2.w + s3.w);
            s.x *= scale; s.y *= scale; s.z *= scale; s.w *= scale;
            *reinterpret_cast<float4*>(out + i) = s;
        } else {
            for (long long e = i; e < count; ++e) {
                float s = slabs[e];
                for (int k = 1; k < nslab; ++k) s += slabs[k * slab_stride + e];
                out[e] = s * scale;
            }
        }
    }
}

// ---- column sums (bias gradients): partial[chunk][n] = sum over the chunk's rows of X[m][n] ------
// HBM-bound (each dZ element read once).  256 threads = 64 column groups (one float4 = 4 columns each,
// so a row segment of 1 KiB is read per 64 lanes) x 4 row lanes; 4 independent loads in flight per thread.
__global__ void __launch_bounds__(256) colsum_partial_kernel(const float* __restrict__ X, int M, int N, int ld, int rows_per_chunk,
                                                            float* __restrict__ partial, long long ldp) {
    __shared__ float4 red[4][64];
    const int cg = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 256 + cg * 4;
    const int r0 = blockIdx.y * rows_per_chunk;
    const int r1 = min(M, r0 + rows_per_chunk);
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
    if (c < N) {
        const float* p = X + c;
        int r = r0 + rl;
        for (; r + 12 < r1; r += 16) {
            const float4 a = *reinterpret_cast<const float4*>(p + (long long)r * ld);
            const float4 b = *reinterpret_cast<const float4*>(p + (long long)(r + 4) * ld);
            const float4 cc = *reinterpret_cast<const float4*>(p + (long long)(r + 8) * ld);
            const float4 d = *reinterpret_cast<const float4*>(p + (long long)(r + 12) * ld);
            s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
            s1.x += b.x; s1.y += b.y; s1.z += b.z; s1.w += b.w;
            s2.x += cc.x; s2.y += cc.y; s2.z += cc.z; s2.w += cc.w;
            s3.x += d.x; s3.y += d.y; s3.z += d.z; s3.w += d.w;
        }
        for (; r < r1; r += 4) {
            const float4 a = *reinterpret_cast<const float4*>(p + (long long)r * ld);
            s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w;
        }
    }
    s0.x += s1.x + s2.x + s3.x; s0.y += s1.y + s2.y + s3.y; s0.z += s1.z + s2.z + s3.z; s0.w += s1.w + s2.w + s3.w;
    red[rl][cg] = s0;
    __syncthreads();
    if (rl == 0 && c < N) {
        const float4 a = red[0][cg], b = red[1][cg], cc = red[2][cg], d = red[3][cg];
        float* o = partial + (long long)blockIdx.y * ldp + c;
        o[0] = a.x + b.x + cc.x + d.x;
        if (c + 1 < N) o[1] = a.y + b.y + cc.y + d.y;
        if (c + 2 < N) o[2] = a.z + b.z + cc.z + d.z;
        if (c + 3 < N) o[3] = a.w + b.w + cc.w + d.w;
    }
}

}  // namespace pulse

using namespace pulse;

namespace {
// Diagnostics state: THREAD-LOCAL (round-3 verdict, hygiene): a tool thread that arms the clock stamps or an occupancy knob changes the
// launches it issues itself, never those of another host thread driving its own stream through the library.
thread_local long long* g_dbg = nullptr;       // tools/gemm_bench --clocks
thread_local int g_last_tile = 0;               // tile rows of the calling thread's last pulse_gemm_f32 launch (pulse_gemm_last_tile: bench.py's per-kernel roofline)
thread_local int g_opt[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // [1] extra LDS bytes per workgroup, [2] no 64-row tile, [3] bf16-storage tile choice (see pulse_hip.h)
}

namespace pulse { int gemm_option(int key) { return key >= 0 && key < 16 ? g_opt[key] : 0; } long long* gemm_debug_buffer() { return g_dbg; } }    // read by gemm_x3p_api.hip (common.h)

namespace {
// Which tiling serves an x3 launch.  Cost model in units of (one 128 x 128 output tile) x (k per split), per CU: the narrow kernel keeps two
// workgroups per CU (a round of 512 costs 2; a lone workgroup per CU 1.5), the wide kernel one workgroup of four tiles' area
// per CU and round at 1.1-1.2 x the narrow kernel's rate on long reductions (about 3.3 units per wide round, more on short ones; calibrated on
// profiles/r05_gemm_x3_wide_ab.txt and on every launch of a cfg2 / cfg3 epoch, profiles/r05_gemm_shapes_cfg{2,3}.txt).  Option 4 (pulse_gemm_set_option) / PULSE_X3_WIDE: 0 automatic, 1 never,
// 2 whenever the output has more than 128 rows and columns (tests).
constexpr int WIDE_TILE = 256;
bool skinny_env_off() { static const bool off = [] { const char* e = getenv("PULSE_X3_SKINNY"); return e && e[0] == '0'; }(); return off; }   // A/B switch, read once
bool g_skinny_unavailable = false;    // the device refused the skinny-N kernel's 144 KB of LDS once
bool g_wide_unavailable = false;      // the device refused the wide tile's LDS request once: never asked again
// 0 = the launcher's cost model, 1 = never the 256 x 256 tile, 2 = whenever the output has more than 128 rows and columns
int x3_mode() {
    static const int env = [] { const char* e = getenv("PULSE_X3_WIDE"); return e ? atoi(e) : -1; }();
    int mode = g_opt[4];
    if (mode == 0 && env >= 0) mode = env == 0 ? 1 : env == 1 ? 0 : env;          // PULSE_X3_WIDE=0 off, 1 automatic, 2 always
    return g_wide_unavailable ? 1 : mode;
}
bool x3_wide_tile(const GemmArgs& g, int lda, int ldb, bool akc, bool bkc) {
    const int mode = x3_mode();
    if (mode == 1 || g.M <= 128 || g.N <= 128) return false;
    // per-workgroup buffer offsets are 32-bit: 256 rows of a reduction-contiguous operand, kchunk rows of a [red][out] operand
    if ((long long)lda * (akc ? 257 : g.kchunk + 1) >= (1LL << 28) || (long long)ldb * (bkc ? 257 : g.kchunk + 1) >= (1LL << 28) ||
        (long long)g.ldc * 257 >= (1LL << 28) || (long long)g.ldaux * 257 >= (1LL << 28))
        return false;
    if (mode == 2) return true;
    const long long z = (long long)g.batch * g.splitk;
    const long long nt = (long long)((g.M + 127) / 128) * ((g.N + 127) / 128) * z;
    const long long wt = (long long)((g.M + 255) / 256) * ((g.N + 255) / 256) * z;
    const long long rem = nt % 512;
    const double cost_narrow = 2.0 * (double)(nt / 512) + (rem == 0 ? 0.0 : rem <= 256 ? 1.5 : 2.0);
    // a round of wide workgroups against a round of 512 narrow ones (= 2 units), from the per-round times of both tilings over the reduction length
    // each workgroup walks (us: narrow 0.0924 k + 5, wide 0.1526 k + f): the wide tile's prologue and epilogue are exposed (one workgroup per CU),
    // f = 8 for plain / ReLU / mask / multiply epilogues, 30 for the SiLU forms that write two outputs and evaluate an exp and a division per
    // element, 45 for the SiLU-derivative epilogue (fits of profiles/r05_gemm_shapes_cfg{2,3}.txt)
    const double kk = (double)g.kchunk < (double)g.K ? (double)g.kchunk : (double)g.K;
    const double fw = g.epi == 2 ? 45.0 : (g.epi == 0 && g.act >= 2) ? 30.0 : 8.0;
    const double wide_round = 2.0 * (0.1526 * kk + fw) / (0.0924 * kk + 5.0);
    const double cost_wide = wide_round * (double)((wt + 255) / 256);
    return cost_wide < cost_narrow;
}
}  // namespace

extern "C" {

int pulse_sizeof_gemm_desc(void) { return (int)sizeof(pulse_gemm_desc); }

int pulse_gemm_set_debug_buffer(long long* device_buffer) { g_dbg = device_buffer; return PULSE_OK; }

int pulse_gemm_last_tile(void) { return g_last_tile; }
int pulse_gemm_x3_mode(void) { return x3_mode(); }

int pulse_gemm_set_option(int key, int value) {
    PULSE_REQUIRE(key >= 0 && key < 16, "pulse_gemm_set_option: bad key");
    g_opt[key] = value;
    return PULSE_OK;
}

int pulse_gemm_f32(const pulse_gemm_desc* d, pulse_stream_t s) {
    PULSE_REQUIRE(d != nullptr, "pulse_gemm_f32: null descriptor");
    PULSE_REQUIRE(d->M >= 0 && d->N >= 0 && d->K >= 0, "pulse_gemm_f32: negative size");
    if (d->M == 0 || d->N == 0 || d->batch == 0) return PULSE_OK;
    PULSE_REQUIRE(d->A && d->B && d->C, "pulse_gemm_f32: null operand");
    PULSE_REQUIRE(d->batch >= 1 && d->split_k >= 1, "pulse_gemm_f32: batch / split_k must be >= 1");
    PULSE_REQUIRE((d->lda % 4) == 0 && (d->ldb % 4) == 0, "pulse_gemm_f32: lda / ldb must be multiples of 4 floats");
    PULSE_REQUIRE((reinterpret_cast<uintptr_t>(d->A) & 15) == 0 && (reinterpret_cast<uintptr_t>(d->B) & 15) == 0,
                  "pulse_gemm_f32: A / B must be 16-byte aligned");
    PULSE_REQUIRE((d->stride_a % 4) == 0 && (d->stride_b % 4) == 0, "pulse_gemm_f32: batch strides must be multiples of 4 floats");
    const bool akc = d->a_layout == PULSE_GEMM_RED_CONTIG, bkc = d->b_layout == PULSE_GEMM_RED_CONTIG;
    PULSE_REQUIRE(!(!akc && bkc), "pulse_gemm_f32: layout combination (A out-contiguous, B reduction-contiguous) unsupported");
    // pitches must cover the float4 reads: reduction-contiguous rows up to roundup4(K), others up to roundup4(extent)
    const int k4 = (d->K + 3) & ~3;
    PULSE_REQUIRE(akc ? d->lda >= k4 : d->lda >= ((d->M + 3) & ~3), "pulse_gemm_f32: lda too small");
    PULSE_REQUIRE(bkc ? d->ldb >= k4 : d->ldb >= ((d->N + 3) & ~3), "pulse_gemm_f32: ldb too small");
    PULSE_REQUIRE(d->ldc >= d->N, "pulse_gemm_f32: ldc too small");
    PULSE_REQUIRE(d->epilogue >= 0 && d->epilogue <= 3 && d->activation >= 0 && d->activation <= 3, "pulse_gemm_f32: bad epilogue / activation");
    PULSE_REQUIRE(d->activation != PULSE_ACT_SILU_D || (d->C2 != nullptr && d->ldc2 >= d->N), "pulse_gemm_f32: ACT_SILU_D stores the derivative in C2");
    PULSE_REQUIRE(d->epilogue == 0 || d->activation == 0, "pulse_gemm_f32: a gradient epilogue takes no activation");
    PULSE_REQUIRE(d->epilogue == 0 || d->aux != nullptr || (d->epilogue == PULSE_EPI_RELU_GRAD && d->relu_mask != nullptr),
                  "pulse_gemm_f32: gradient epilogue needs aux (or, for relu-grad, relu_mask)");
    const bool mask_on = d->relu_mask != nullptr && ((d->epilogue == PULSE_EPI_RELU_GRAD && d->aux == nullptr) ||
                                                     (d->epilogue == PULSE_EPI_BIAS_ACT && d->activation == PULSE_ACT_RELU));
    PULSE_REQUIRE(!mask_on || (d->ld_mask >= (d->N + 3) / 4 && d->split_k == 1), "pulse_gemm_f32: relu_mask needs ld_mask >= roundup4(N) / 4 and no split-K");
    PULSE_REQUIRE(d->rowsum == nullptr || (!akc && !bkc), "pulse_gemm_f32: rowsum needs the (OUT, OUT) layouts (dW pass)");
    PULSE_REQUIRE(d->split_k == 1 || (d->epilogue == 0 && d->activation == 0 && d->bias == nullptr),
                  "pulse_gemm_f32: split-K slabs carry no epilogue");

    GemmArgs g;
    g.A = d->A; g.B = d->B; g.C = d->C; g.C2 = d->C2; g.bias = d->bias; g.aux = d->aux;
    g.M = d->M; g.N = d->N; g.K = d->K;
    g.lda = d->lda; g.ldb = d->ldb; g.ldc = d->ldc; g.ldc2 = d->ldc2; g.ldaux = d->ldaux;
    g.sA = d->stride_a; g.sB = d->stride_b; g.sC = d->stride_c; g.sC2 = d->stride_c2; g.sBias = d->stride_bias; g.sAux = d->stride_aux;
    g.batch = d->batch; g.splitk = d->split_k;
    const int bk = d->compute_type == PULSE_GEMM_COMPUTE_BF16 ? BK16 : d->compute_type == PULSE_GEMM_COMPUTE_F32X3 ? XK : BK;
    int kchunk = (d->K + d->split_k - 1) / d->split_k;
    kchunk = ((kchunk + bk - 1) / bk) * bk;
    g.kchunk = kchunk > 0 ? kchunk : bk;
    g.sSplit = d->split_stride;
    g.act = d->activation; g.epi = d->epilogue;
    g.rowsum = d->rowsum; g.sRowsum = d->stride_rowsum;
    g.mask = mask_on ? d->relu_mask : nullptr; g.ldmask = d->ld_mask; g.sMask = d->stride_mask;
    g.tiles_m = (d->M + BM - 1) / BM; g.tiles_n = (d->N + BN - 1) / BN;
    // x3 only: a 64-row tile for skinny outputs (one column tile: the mu / value heads) whose 128-row tiling leaves the chip at one
    // workgroup per CU or less.  Measured: heads at M = 16384 36.2 -> 32.8 us, at M = 4096 28.5 -> 21.6 us; full-width outputs at the same
    // workgroup count get SLOWER with the half tile (twice the B staging per MFMA: rollout layer 2 52.8 -> 58.3 us), so they keep 128 rows.
    const bool half_tile = d->compute_type == PULSE_GEMM_COMPUTE_F32X3 && d->M >= 256 && g.tiles_n == 1 &&
                           (long long)g.tiles_m * d->batch * d->split_k < 384 && g_opt[2] == 0;
    if (half_tile) g.tiles_m = (d->M + 63) / 64;
    g.dbg = g_dbg;
    PULSE_REQUIRE(d->compute_type == PULSE_GEMM_COMPUTE_F32 || d->compute_type == PULSE_GEMM_COMPUTE_BF16 ||
                  d->compute_type == PULSE_GEMM_COMPUTE_F32X3, "pulse_gemm_f32: bad compute_type");
    const bool bf = d->compute_type == PULSE_GEMM_COMPUTE_BF16, x3 = d->compute_type == PULSE_GEMM_COMPUTE_F32X3;
    g.round_bf16 = bf && d->round_output_bf16 ? 1 : 0;
    // per-workgroup buffer offsets are 32-bit: tile-relative (128 rows) for reduction-contiguous operands, split-relative
    // (kchunk rows) for [red][out] operands
    PULSE_REQUIRE((long long)d->lda * (akc ? 129 : g.kchunk + 1) < (1LL << 28) && (long long)d->ldb * (bkc ? 129 : g.kchunk + 1) < (1LL << 28) &&
                  (long long)d->ldc * 129 < (1LL << 28) && (long long)d->ldaux * 129 < (1LL << 28),
                  "pulse_gemm_f32: pitch too large for 32-bit tile-relative offsets");
    auto al16 = [](const void* p, long long ld, long long st) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld % 4) == 0 && (st % 4) == 0; };
    g.vec_epi = al16(d->C, d->ldc, d->stride_c) && (d->split_stride % 4) == 0 && (!d->aux || al16(d->aux, d->ldaux, d->stride_aux)) &&
                (!d->C2 || al16(d->C2, d->ldc2, d->stride_c2)) && (!d->bias || al16(d->bias, 4, d->stride_bias));
    PULSE_REQUIRE(!mask_on || g.vec_epi, "pulse_gemm_f32: relu_mask needs 16-byte aligned C / pitches (a lane owns four columns of a mask word)");
    g_last_tile = half_tile ? 64 : 128;
    // skinny outputs over a long M (the mu / value heads, the latent-width layers): gemm_x3s.hip -- a workgroup owns 128 rows x all N <= 96
    // columns, A goes global -> registers -> fragments, B is split once per workgroup and 128-deep k phase.  Bit-identical to the other tilings.
    // Taken when the launch is ONE round of 128-row workgroups that fills most of the chip (192 .. 256 of them; measured, tools/bench_gemm_x3_skinny.py:
    // 16384 x 69 x 512 x 2 nets 34.2 -> 29.1 us, but two rounds (32768 rows) 47.7 -> 57.9 and half a round no gain); gemm option 6 = 1: never.
    if (x3 && akc && d->N <= 96 && d->epilogue == PULSE_EPI_BIAS_ACT && d->activation <= PULSE_ACT_RELU && d->C2 == nullptr && d->split_k == 1 &&
        d->rowsum == nullptr && !mask_on && g_dbg == nullptr && g_opt[6] == 0 && !g_skinny_unavailable && !skinny_env_off() &&
        (long long)((d->M + 127) / 128) * d->batch >= 192 && (long long)((d->M + 127) / 128) * d->batch <= 256 && (long long)d->lda * 129 < (1LL << 28) &&
        (bkc ? (long long)d->ldb * 97 : (long long)d->ldb * (d->K + 1)) < (1LL << 28)) {
        const int rc = launch_gemm_x3s(g, bkc, as_stream(s));
        if (rc != kWideTileUnavailable) { g_last_tile = 96; return rc; }
        g_skinny_unavailable = true;
    }
    if (x3 && !half_tile && x3_wide_tile(g, d->lda, d->ldb, akc, bkc)) {
        // 256 x 256 tile (gemm_x3w.hip): half the split / staging work per MFMA; taken when its one-workgroup-per-CU rounds cost less than the
        // 128 x 128 tiling's (two workgroups per CU) -- see x3_wide_tile.  A device that does not grant its 135 KB of LDS keeps the narrow tile
        // (same bits either way).
        // A narrow column tail that costs the wide tiling a whole extra round of workgroups (N = 3096 = 12 x 256 + 24: 13 column tiles, 832
        // workgroups = 4 rounds at M = 16384, where 12 x 64 = 768 is exactly 3) goes to the 128 x 128 tiling as a launch of its own: the two
        // tilings are bit-identical, so the split is invisible in the results.  (Epilogue-carrying launches only: a split-K / row-sum launch
        // writes slabs whose tiling the planner already sized.)
        const int ntail = d->N % WIDE_TILE;
        if (ntail > 0 && ntail <= 64 && d->N > WIDE_TILE && d->split_k == 1 && d->rowsum == nullptr && g_opt[5] == 0) {
            const long long tm = (d->M + WIDE_TILE - 1) / WIDE_TILE, z = d->batch;
            const long long r_all = (tm * ((d->N + WIDE_TILE - 1) / WIDE_TILE) * z + 255) / 256, r_main = (tm * (d->N / WIDE_TILE) * z + 255) / 256;
            if (r_main < r_all) {
                const int n0 = d->N - ntail;
                pulse_gemm_desc m = *d, t = *d;
                m.N = n0;
                t.N = ntail;
                t.B = bkc ? d->B + (long long)n0 * d->ldb : d->B + n0;
                t.C = d->C + n0;
                if (d->C2) t.C2 = d->C2 + n0;
                if (d->bias) t.bias = d->bias + n0;
                if (d->aux) t.aux = d->aux + n0;
                if (d->relu_mask) t.relu_mask = d->relu_mask + n0 / 4;
                const int rc_main = pulse_gemm_f32(&m, s);
                if (rc_main != PULSE_OK) return rc_main;
                const int rc_tail = pulse_gemm_f32(&t, s);
                g_last_tile = 256;                                   // (diagnostics: the launch's time is the wide kernel's)
                return rc_tail;
            }
        }
        const int rc = launch_gemm_x3w(g, akc, bkc, as_stream(s));
        if (rc != kWideTileUnavailable) { g_last_tile = 256; return rc; }
        g_wide_unavailable = true;
    }
    const size_t extra_lds = (size_t)g_opt[1];
    if (x3) return launch_gemm_x3(g, akc, bkc, half_tile, extra_lds, as_stream(s));
    if (bf) return launch_gemm_bf16c(g, akc, bkc, extra_lds, as_stream(s));
    return launch_gemm_mfma32(g, akc, bkc, extra_lds, as_stream(s));
}

int pulse_reduce_slabs(const float* slabs, int32_t num_slabs, int64_t slab_stride, int64_t count, float* out, float scale,
                       pulse_stream_t s) {
    PULSE_REQUIRE(num_slabs >= 1 && count >= 0, "pulse_reduce_slabs: bad sizes");
    if (count == 0) return PULSE_OK;
    PULSE_REQUIRE(slabs && out, "pulse_reduce_slabs: null pointer");
    PULSE_REQUIRE((slab_stride % 4) == 0 && (reinterpret_cast<uintptr_t>(slabs) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0,
                  "pulse_reduce_slabs: 16-byte alignment required");
    long long blocks = (count / 4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(s), slabs, num_slabs, slab_stride, count, out, scale);
    return check_launch("pulse_reduce_slabs");
}

int pulse_colsum_partial(const float* x, int32_t m, int32_t n, int32_t ld, int32_t num_chunks, float* partial, int64_t ld_partial,
                         pulse_stream_t s) {
    PULSE_REQUIRE(m >= 0 && n >= 0 && num_chunks >= 1, "pulse_colsum_partial: bad sizes");
    if (n == 0) return PULSE_OK;
    PULSE_REQUIRE(x && partial && ld >= ((n + 3) & ~3) && ld_partial >= n, "pulse_colsum_partial: bad pointers / pitches (ld must cover roundup4(n))");
    PULSE_REQUIRE((ld % 4) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0, "pulse_colsum_partial: x rows must be 16-byte aligned");
    const int rows = (m + num_chunks - 1) / num_chunks;
    hipLaunchKernelGGL(colsum_partial_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)num_chunks), dim3(256), 0, as_stream(s), x, m, n, ld,
                       rows > 0 ? rows : 1, partial, (long long)ld_partial);
    return check_launch("pulse_colsum_partial");
}
}
