// FP32 MFMA GEMM for the actor / critic / VAE MLPs (forward, dX and dW passes) on gfx950.
//
// Replaces every nn.Linear call (+ its autograd backward) on the PPO update path:
//   phc/learning/network_builder.py:105-124,245-261 (actor_mlp / critic_mlp / mu / value),
//   phc/learning/amp_network_builder.py:127-148,206-211 (eval_actor / eval_critic),
//   phc/learning/amp_network_z_builder.py:469-580 (PULSE VAE encoder / prior / decoder MLPs).
//
// Arithmetic: v_mfma_f32_32x32x2_f32 -- f32 inputs, f32 accumulate, bit-identical to an fmaf chain,
// 64 FLOP/clk/SIMD (157 TFLOP/s chip peak at 2.4 GHz; gfx950 has no TF32/xf32 path).  The reference trains in
// fp32 (mixed_precision: False, learning/im.yaml:50), so fp32 is kept end to end.
//
// One kernel, three operand-layout instantiations, C[m][n] = sum_k A(m,k) * B(n,k):
//   <KC,KC>  forward   Y = X W^T      X [M][K],  W [N][K]      (both reduction-contiguous)
//   <KC,MC>  dX        dX = dY W      dY [M][N], W [N][K]      (B stored [red][out])
//   <MC,MC>  dW        dW = dY^T X    dY [M][N], X [M][K]      (both stored [red][out], split-K over M)
// Tiling: 128x128x32 block tile, 4 waves (2x2), each wave 2x2 MFMA tiles of 32x32 (64 accumulator registers), two
// workgroups per CU (LDS-limited), so every SIMD holds two waves that fill each other's stalls.
//
// What the round-2 measurements (tools/gemm_bench --clocks: per-workgroup s_memtime stamps) said, and what this
// version does about it:
//   * beside an fp32-MFMA-saturating partner wave every VALU instruction of the other wave waits for a gap between
//     two 64-cycle MFMAs, and every VALU instruction of the MFMA wave itself delays its next MFMA: VALU work is the
//     scarce resource.  The old epilogue (~400 VALU per wave) took 29k cycles per tile beside a busy partner (9.8k
//     alone) and the dW main loop lost 14 % to bias-gradient adds and address arithmetic.
//   * so: global loads are buffer loads (per-lane byte offset computed ONCE, the k advance rides in the scalar
//     offset), LDS addresses are per-lane constants + immediates (the LDS stage is a template parameter), the
//     reduction-tail masks exist only in the tile that stages the last k-tile, the bias is the initial value of the
//     accumulators, the fast epilogue is ds_write / ds_read_b128 / activation / buffer_store with scalar row offsets.
//   * ONE LDS image for all layouts, [k-chunk of 4][out][4 k] in 16-byte slots, 129 slots per k-chunk block, slot =
//     out ^ ((out >> 3) & 7): reduction-contiguous operands are stored as loaded, [red][out] operands are transposed
//     4x4 in registers on the way in, and every fragment is one conflict-free ds_read_b128 feeding four MFMAs (k is a
//     pure reduction index, so the two wave halves take k-chunks 2g and 2g+1 of every 8-k group, A and B alike).
// 256 CUs / 8 XCDs: the 1-D grid is remapped so each XCD owns a contiguous band of m-tiles (A panels stay in that
// XCD's L2; the small weight matrix is shared by all).
#include <type_traits>
#include "common.h"
#include "gemm_shared.h"
#include "gemm_epilogue.h"

namespace pulse {

constexpr int KC_SLOTS = 129;                        // 16-byte slots per k-chunk block: 128 outs + 1 pad slot
constexpr int IMG_BYTES = 8 * KC_SLOTS * 16;         // one operand tile: 8 k-chunks x 129 slots = 16,512 B
constexpr int STAGE_BYTES = 2 * IMG_BYTES;           // A image + B image
constexpr int LDS_BYTES = 2 * STAGE_BYTES;           // two stages = 66,048 B -> two workgroups per CU

// Per-thread staging state of one operand: 4 in-flight 16-byte loads, their (constant) buffer byte offsets and the
// (constant) LDS byte addresses their data goes to.
//   KC (reduction-contiguous): load i = row (tid >> 3) + 32 i, k-chunk tid & 7      -> one slot, stored as loaded
//   MC ([red][out]):           load i = k row 4 (tid >> 5) + i, outs 4 (tid & 31).. -> 4x4 transpose, store j = out 4L + j
template <bool KC>
struct Stager {
    f32x4 r[4];
    int voff[4];
    int lds[4];
    int kpos;            // KC: first k of this thread's slot inside the tile (0, 4, .. 28); MC: first k row (0, 4, .. 28)

    __device__ __forceinline__ void init(int tid, int ld, int ext_rel /* valid outs from the tile origin, >= 1 */, int img_off) {
        if constexpr (KC) {
            const int kc = tid & 7, row0 = tid >> 3;
            kpos = kc * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + 32 * i;
                const int rr = row < ext_rel ? row : ext_rel - 1;       // rows beyond the extent are never stored: read a valid one
                voff[i] = (rr * ld + kc * 4) * 4;
                lds[i] = img_off + (kc * KC_SLOTS + slot_of(row)) * 16;
            }
        } else {
            const int kch = tid >> 5, L = tid & 31;
            kpos = kch * 4;
            const int col = 4 * L < ext_rel ? 4 * L : 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                voff[i] = ((kch * 4 + i) * ld + col) * 4;
                lds[i] = img_off + (kch * KC_SLOTS + slot_of(4 * L + i)) * 16;
            }
        }
    }
    // single short tile (K < 32 from the window start): lanes past the readable range re-read k position 0 (masked later)
    __device__ __forceinline__ void clamp_short(int tid, int ld, int readable /* k positions that may be read */) {
        if constexpr (KC) {
            if (kpos >= readable) {
#pragma unroll
                for (int i = 0; i < 4; ++i) voff[i] -= kpos * 4;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (kpos + i >= readable) voff[i] -= (kpos + i) * ld * 4;
        }
    }
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rs, int soff, int i) { r[i] = buf_load(rs, voff[i], soff); }

    // store unit u (0..3) into the stage at byte offset st; MASKED zeroes k positions outside [lo, hi)
    template <bool MASKED>
    __device__ __forceinline__ void store(int st, int u, int lo, int hi) {
        if constexpr (KC) {
            f32x4 v = r[u];
            if constexpr (MASKED) {
                if (kpos < lo || kpos >= hi) v.x = 0.f;
                if (kpos + 1 < lo || kpos + 1 >= hi) v.y = 0.f;
                if (kpos + 2 < lo || kpos + 2 >= hi) v.z = 0.f;
                if (kpos + 3 < lo || kpos + 3 >= hi) v.w = 0.f;
            }
            lds_write(st + lds[u], v);
        } else {
            f32x4 v = {r[0][u], r[1][u], r[2][u], r[3][u]};            // out 4L + u, k rows kpos .. kpos + 3
            if constexpr (MASKED) {
                if (kpos < lo || kpos >= hi) v.x = 0.f;
                if (kpos + 1 < lo || kpos + 1 >= hi) v.y = 0.f;
                if (kpos + 2 < lo || kpos + 2 >= hi) v.z = 0.f;
                if (kpos + 3 < lo || kpos + 3 >= hi) v.w = 0.f;
            }
            lds_write(st + lds[u], v);
        }
    }
};

template <bool AKC, bool BKC>
__global__ void __launch_bounds__(256) gemm_f32_kernel(const GemmArgs g) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5;
    const int l31 = lane & 31;

    // XCD-aware workgroup order (map_workgroup above): a band of output tiles per XCD, or a k range per XCD for split-K launches
    const WgMap wg = map_workgroup(g.tiles_m * g.tiles_n, g.batch, g.splitk);
    const int id = wg.id;
    const int tm = id / g.tiles_n, tn = id - tm * g.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int bz = wg.bz, sp = wg.sp;
    const int kbeg = sp * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const int klen = kend - kbeg;
    const int nkt = (klen + BK - 1) / BK;

    long long dbg_c0 = 0, dbg_w0 = 0, dbg_c1 = 0, dbg_w1 = 0;
    if (g.dbg) { dbg_c0 = clock64(); dbg_w0 = wall_clock64(); }

    // The last k-tile is read through a window that ENDS at roundup4(kend) (never past a row's pitch / the last k row):
    // it may overlap the tile before it, so its image is valid for positions [lo, hi) only.
    const int r4 = (klen + 3) & ~3;
    const int wlast = r4 > BK ? r4 - BK : 0;                 // window start of the last tile, relative to kbeg
    const int lo = nkt > 0 ? (nkt - 1) * BK - wlast : 0;
    const int hi = klen - wlast;

    // buffer resources based at this workgroup's tile origin and k start (all offsets stay far below 2^31)
    const float* Ab = g.A + bz * g.sA + (AKC ? (long long)m0 * g.lda + kbeg : (long long)kbeg * g.lda + m0);
    const float* Bb = g.B + bz * g.sB + (BKC ? (long long)n0 * g.ldb + kbeg : (long long)kbeg * g.ldb + n0);
    // [red][out] operands: the shifted window of the last k-tile may name up to three k rows past the operand's last row; the buffer
    // extent makes those loads return zero without touching memory (they are masked anyway)
    const unsigned recA = AKC ? 0xffffffffu : (unsigned)((g.K - kbeg - 1) * g.lda + ((min(BM, g.M - m0) + 3) & ~3)) * 4u;
    const unsigned recB = BKC ? 0xffffffffu : (unsigned)((g.K - kbeg - 1) * g.ldb + ((min(BN, g.N - n0) + 3) & ~3)) * 4u;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Ab), 0, recA, RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Bb), 0, recB, RSRC_FLAGS);
    const int kstepA = AKC ? 4 : g.lda * 4, kstepB = BKC ? 4 : g.ldb * 4;        // bytes per unit of k
    auto koff = [&](int t) { return t == nkt - 1 ? wlast : t * BK; };              // scalar

    Stager<AKC> sa;
    Stager<BKC> sb;
    sa.init(tid, g.lda, g.M - m0, 0);
    sb.init(tid, g.ldb, g.N - n0, IMG_BYTES);
    if (nkt == 1 && r4 < BK) { sa.clamp_short(tid, g.lda, AKC ? r4 : klen); sb.clamp_short(tid, g.ldb, BKC ? r4 : klen); }

    // fragment read addresses: lane (l31, half) reads out (wm|wn) * 64 + {0, 32} + l31, k-chunk 2g + half
    const int frA0 = (half * KC_SLOTS + slot_of(wm * 64 + l31)) * 16;
    const int frA1 = (half * KC_SLOTS + slot_of(wm * 64 + 32 + l31)) * 16;
    const int frB0 = IMG_BYTES + (half * KC_SLOTS + slot_of(wn * 64 + l31)) * 16;
    const int frB1 = IMG_BYTES + (half * KC_SLOTS + slot_of(wn * 64 + 32 + l31)) * 16;

    // accumulators start from the bias (EPI 0): the epilogue has no bias add left
    f32x16 acc[2][2];
    {
        float b0 = 0.f, b1 = 0.f;
        if (g.epi == 0 && g.bias) {
            const float* bias = g.bias + bz * g.sBias;
            const int c0 = n0 + wn * 64 + l31;
            if (c0 < g.N) b0 = bias[c0];
            if (c0 + 32 < g.N) b1 = bias[c0 + 32];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][0][r] = b0; acc[i][1][r] = b1; }
    }

    f32x4 fa[2][2], fb[2][2];                                    // two fragment sets: one feeding MFMAs, one in flight from LDS
    float rsum[2] = {0.f, 0.f};
    const bool do_rs = !AKC && g.rowsum != nullptr && tn == 0 && wn == 0;      // wave-uniform

    // fragment unit u of set SET for k-group G of the stage at byte offset ST: order fa0, fb0, fb1, fa1 = consumption order
    auto frag_unit = [&](int set, int u, int st, int G) {
        const int o = st + 2 * G * KC_SLOTS * 16;
        if (u == 0) fa[set][0] = lds_read(frA0 + o);
        else if (u == 1) fb[set][0] = lds_read(frB0 + o);
        else if (u == 2) fb[set][1] = lds_read(frB1 + o);
        else fa[set][1] = lds_read(frA1 + o);
    };

    // One k-tile = 64 MFMAs issued as 32 PAIRS (two accumulator chains alternate, so no MFMA waits on its predecessor);
    // after every pair exactly one small unit of side work (none of them VALU in the steady state for KC operands):
    //   pairs  0-3   fragment reads for pairs  8-15   (set 1, k-group 1)
    //   pairs  8-11  fragment reads for pairs 16-23   (set 0, k-group 2)
    //   pairs 16-19  fragment reads for pairs 24-31   (set 1, k-group 3)
    //   pairs 19-26  the 8 register->LDS stores of tile t+1 (its global loads were issued a tile ago)
    //   after pair 27  the ONE barrier of the tile
    //   pairs 24-31  the 8 buffer loads of tile t+2 (load k re-uses the registers store k just drained; A's four stores
    //                are done by pair 22, B's by pair 26)
    //   pairs 28-31  fragment reads for pairs 0-7 of tile t+1 (set 0, other LDS stage)
    // MODE 0 steady, 1 = stages the LAST tile (masked stores, no further loads), 2 = last tile (compute only).
    auto tile = [&](auto mode_tag, auto stage_tag, int t) {
        constexpr int MODE = decltype(mode_tag)::value;
        constexpr int CUR = decltype(stage_tag)::value * STAGE_BYTES, OTH = STAGE_BYTES - CUR;
        const int soA = koff(t + 2) * kstepA, soB = koff(t + 2) * kstepB;
#pragma unroll
        for (int p = 0; p < 32; ++p) {
            const int grp = p >> 3, set = grp & 1, q = p & 7, i = q >> 2, c = q & 3;
            if constexpr (!AKC) {                  // dW pass: the A fragments are dY -- their k-sums are the bias gradient
                if (q == 0 && do_rs) {
                    rsum[0] += (fa[set][0].x + fa[set][0].y) + (fa[set][0].z + fa[set][0].w);
                    rsum[1] += (fa[set][1].x + fa[set][1].y) + (fa[set][1].z + fa[set][1].w);
                }
            }
            acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][i][c], fb[set][0][c], acc[i][0], 0, 0, 0);
            acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][i][c], fb[set][1][c], acc[i][1], 0, 0, 0);
            if (p < 4) frag_unit(1, p, CUR, 1);
            else if (p >= 8 && p < 12) frag_unit(0, p - 8, CUR, 2);
            else if (p >= 16 && p < 20) frag_unit(1, p - 16, CUR, 3);
            if constexpr (MODE != 2) {
                if (p >= 19 && p < 27) {
                    const int u = p - 19;
                    if (u < 4) sa.template store<MODE == 1>(OTH, u, lo, hi);
                    else sb.template store<MODE == 1>(OTH, u - 4, lo, hi);
                }
                if (p == 27) {
                    __builtin_amdgcn_sched_barrier(0);
                    __syncthreads();
                }
                if constexpr (MODE == 0) {
                    if (p >= 24) {
                        const int u = p - 24;
                        if (u < 4) sa.load(rsA, soA, u);
                        else sb.load(rsB, soB, u - 4);
                    }
                }
                if (p >= 28) frag_unit(0, p - 28, OTH, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;

    if (nkt > 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) { sa.load(rsA, koff(0) * kstepA, u); sb.load(rsB, koff(0) * kstepB, u); }
        if (nkt == 1) {
#pragma unroll
            for (int u = 0; u < 4; ++u) { sa.template store<true>(0, u, lo, hi); sb.template store<true>(0, u, lo, hi); }
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) { sa.template store<false>(0, u, 0, BK); sb.template store<false>(0, u, 0, BK); }
        }
    }
    __syncthreads();
    if (nkt > 1) {
#pragma unroll
        for (int u = 0; u < 4; ++u) { sa.load(rsA, koff(1) * kstepA, u); sb.load(rsB, koff(1) * kstepB, u); }
    }
    if (nkt > 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) frag_unit(0, u, 0, 0);
    }
    {
        int t = 0;
        for (; t + 3 < nkt; t += 2) { tile(I0{}, I0{}, t); tile(I0{}, I1{}, t + 1); }      // steady tiles t < nkt - 2, two per trip
        if (t + 2 < nkt) {                                                               // one more steady tile: parity flips
            tile(I0{}, I0{}, t);
            tile(I1{}, I1{}, t + 1);
            tile(I2{}, I0{}, t + 2);
        } else if (t + 2 == nkt) {
            tile(I1{}, I0{}, t);
            tile(I2{}, I1{}, t + 1);
        } else if (t + 1 == nkt) {
            tile(I2{}, I0{}, t);
        }
    }
    if constexpr (!AKC) {
        if (do_rs) {
            // this lane summed the k-chunks of its half; the other half's lane holds the rest of the same row
            const float r0 = rsum[0] + __shfl_xor(rsum[0], 32, 64);
            const float r1 = rsum[1] + __shfl_xor(rsum[1], 32, 64);
            if (half == 0) {
                float* rs = g.rowsum + bz * g.sRowsum + sp * g.sSplit;
                const int row = m0 + wm * 64 + l31;
                if (row < g.M) rs[row] = r0;
                if (row + 32 < g.M) rs[row + 32] = r1;
            }
        }
    }
    __syncthreads();                                              // the epilogue reuses the staging buffers
    if (g.dbg) { dbg_c1 = clock64(); dbg_w1 = wall_clock64(); }
    struct DbgStamp {
        const GemmArgs& g; long long c0, w0, c1, w1;
        __device__ ~DbgStamp() {
            if (g.dbg && threadIdx.x == 0) {
                long long* o = g.dbg + 8 * (blockIdx.y * gridDim.x + blockIdx.x);
                o[0] = c0; o[1] = w0; o[2] = c1; o[3] = w1; o[4] = clock64(); o[5] = wall_clock64();
                o[7] = ((long long)__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) << 32) | (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);
            }
        }
    } dbg_stamp{g, dbg_c0, dbg_w0, dbg_c1, dbg_w1};

    gemm_epilogue(g, acc, tid, m0, n0, bz, sp, wm, wn, half, l31);
}

// =====================================================================================================================
// bf16 MFMA variant (BASELINE.json configs[4]: "AMP discriminator + PPO ... bf16"; the reference's autocast site is
// phc/learning/amp_agent.py:671, common_agent.py:426,461).  Storage stays fp32 (fp32 master weights, fp32 activations in HBM);
// operands are rounded to bf16 ON THE WAY INTO LDS, products accumulate in fp32 on v_mfma_f32_32x32x16_bf16 (16x the fp32 MFMA
// rate), and with round_bf16 the outputs leave as bf16-representable values -- exactly what a bf16 autocast Linear computes.
// Same 128x128 tile, same LDS image geometry with 8 bf16 per 16-byte slot, so one k-tile is 64 deep and one ds_read_b128 is the
// whole operand of one MFMA.  At this MFMA rate the kernel is bound by the fp32 operand traffic (L2 / HBM), not by the matrix pipe:
// a plain double-buffered loop, all fragment reads of a stage issued before the tile's barrier (same race rule as above).
// =====================================================================================================================

__device__ __forceinline__ bf16x8 pack8(const float (&v)[8]) {
    bf16x8 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bf16x2 t = __builtin_convertvector((f32x2){v[2 * k], v[2 * k + 1]}, bf16x2);
        o[2 * k] = t[0]; o[2 * k + 1] = t[1];
    }
    return o;
}

template <bool KC>
struct Stager16 {
    f32x4 r[8];
    int voff[8];         // KC: 4 used (each slot = two adjacent 16-byte loads); MC: 8 k rows
    int lds[4];
    int kpos;            // first k position of this thread's slot(s) inside the 64-deep tile

    __device__ __forceinline__ void init(int tid, int ld, int ext_rel, int img_off) {
        if constexpr (KC) {
            const int kc = tid & 7, row0 = tid >> 3;
            kpos = kc * 8;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + 32 * i;
                const int rr = row < ext_rel ? row : ext_rel - 1;
                voff[i] = (rr * ld + kc * 8) * 4;
                lds[i] = img_off + (kc * KC_SLOTS + slot_of(row)) * 16;
            }
        } else {
            const int kch = tid >> 5, L = tid & 31;
            kpos = kch * 8;
            const int col = 4 * L < ext_rel ? 4 * L : 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) voff[i] = ((kch * 8 + i) * ld + col) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) lds[j] = img_off + (kch * KC_SLOTS + slot_of(4 * L + j)) * 16;
        }
    }
    __device__ __forceinline__ void clamp_short(int ld, int readable) {
        if constexpr (KC) {
            // a 16-byte load covers 4 k positions: the first half is readable if kpos < readable, the second if kpos + 4 < readable
            if (kpos >= readable) {                                  // nothing of this slot is readable: both halves re-read position 0
#pragma unroll
                for (int i = 0; i < 4; ++i) voff[i] -= kpos * 4;
                kpos_hi_ok = false;
            } else {
                kpos_hi_ok = kpos + 4 < readable;                     // second half past the readable range: re-read the first half
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (kpos + i >= readable) voff[i] -= (kpos + i) * ld * 4;
        }
    }
    bool kpos_hi_ok = true;
    __device__ __forceinline__ void load_all(__amdgpu_buffer_rsrc_t rs, int soff) {
        if constexpr (KC) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                r[2 * i] = buf_load(rs, voff[i], soff);
                r[2 * i + 1] = buf_load(rs, voff[i] + (kpos_hi_ok ? 16 : 0), soff);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] = buf_load(rs, voff[i], soff);
        }
    }
    template <bool MASKED>
    __device__ __forceinline__ void store(int st, int u, int lo, int hi) {
        float v[8];
        if constexpr (KC) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = r[2 * u][e]; v[4 + e] = r[2 * u + 1][e]; }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = r[i][u];
        }
        if constexpr (MASKED) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (kpos + e < lo || kpos + e >= hi) v[e] = 0.f;
        }
        extern __shared__ __attribute__((aligned(16))) char smem_c[];
        *reinterpret_cast<bf16x8*>(smem_c + st + lds[u]) = pack8(v);
    }
};

template <bool AKC, bool BKC>
__global__ void __launch_bounds__(256) gemm_bf16_kernel(const GemmArgs g) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5;
    const int l31 = lane & 31;
    const WgMap wg = map_workgroup(g.tiles_m * g.tiles_n, g.batch, g.splitk);
    const int id = wg.id;
    const int tm = id / g.tiles_n, tn = id - tm * g.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int bz = wg.bz, sp = wg.sp;
    const int kbeg = sp * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const int klen = kend - kbeg;
    const int nkt = (klen + BK16 - 1) / BK16;
    const int r4 = (klen + 3) & ~3;
    const int wlast = r4 > BK16 ? r4 - BK16 : 0;
    const int lo = nkt > 0 ? (nkt - 1) * BK16 - wlast : 0;
    const int hi = klen - wlast;

    const float* Ab = g.A + bz * g.sA + (AKC ? (long long)m0 * g.lda + kbeg : (long long)kbeg * g.lda + m0);
    const float* Bb = g.B + bz * g.sB + (BKC ? (long long)n0 * g.ldb + kbeg : (long long)kbeg * g.ldb + n0);
    // [red][out] operands: the shifted window of the last k-tile may name up to three k rows past the operand's last row; the buffer
    // extent makes those loads return zero without touching memory (they are masked anyway)
    const unsigned recA = AKC ? 0xffffffffu : (unsigned)((g.K - kbeg - 1) * g.lda + ((min(BM, g.M - m0) + 3) & ~3)) * 4u;
    const unsigned recB = BKC ? 0xffffffffu : (unsigned)((g.K - kbeg - 1) * g.ldb + ((min(BN, g.N - n0) + 3) & ~3)) * 4u;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Ab), 0, recA, RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Bb), 0, recB, RSRC_FLAGS);
    const int kstepA = AKC ? 4 : g.lda * 4, kstepB = BKC ? 4 : g.ldb * 4;
    auto koff = [&](int t) { return t == nkt - 1 ? wlast : t * BK16; };

    Stager16<AKC> sa;
    Stager16<BKC> sb;
    sa.init(tid, g.lda, g.M - m0, 0);
    sb.init(tid, g.ldb, g.N - n0, IMG_BYTES);
    if (nkt == 1 && r4 < BK16) { sa.clamp_short(g.lda, AKC ? r4 : klen); sb.clamp_short(g.ldb, BKC ? r4 : klen); }

    const int frA0 = (half * KC_SLOTS + slot_of(wm * 64 + l31)) * 16;
    const int frA1 = (half * KC_SLOTS + slot_of(wm * 64 + 32 + l31)) * 16;
    const int frB0 = IMG_BYTES + (half * KC_SLOTS + slot_of(wn * 64 + l31)) * 16;
    const int frB1 = IMG_BYTES + (half * KC_SLOTS + slot_of(wn * 64 + 32 + l31)) * 16;

    f32x16 acc[2][2];
    {
        float b0 = 0.f, b1 = 0.f;
        if (g.epi == 0 && g.bias) {
            const float* bias = g.bias + bz * g.sBias;
            const int c0 = n0 + wn * 64 + l31;
            if (c0 < g.N) b0 = bias[c0];
            if (c0 + 32 < g.N) b1 = bias[c0 + 32];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][0][r] = b0; acc[i][1][r] = b1; }
    }
    float rsum[2] = {0.f, 0.f};
    const bool do_rs = !AKC && g.rowsum != nullptr && tn == 0 && wn == 0;

    bf16x8 fa[4][2], fb[4][2];                                     // the four 16-k groups of one tile
    auto frags = [&](int G, int st) {
        extern __shared__ __attribute__((aligned(16))) char smem_c[];
        const int o = st + 2 * G * KC_SLOTS * 16;
        fa[G][0] = *reinterpret_cast<const bf16x8*>(smem_c + frA0 + o);
        fb[G][0] = *reinterpret_cast<const bf16x8*>(smem_c + frB0 + o);
        fb[G][1] = *reinterpret_cast<const bf16x8*>(smem_c + frB1 + o);
        fa[G][1] = *reinterpret_cast<const bf16x8*>(smem_c + frA1 + o);
    };
    auto mma = [&](int G) {
        if constexpr (!AKC) {
            if (do_rs) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { rsum[0] += (float)fa[G][0][e]; rsum[1] += (float)fa[G][1][e]; }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[G][i], fb[G][0], acc[i][0], 0, 0, 0);
            acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[G][i], fb[G][1], acc[i][1], 0, 0, 0);
        }
    };

    if (nkt > 0) {
        sa.load_all(rsA, koff(0) * kstepA);
        sb.load_all(rsB, koff(0) * kstepB);
        if (nkt == 1) {
#pragma unroll
            for (int u = 0; u < 4; ++u) { sa.template store<true>(0, u, lo, hi); sb.template store<true>(0, u, lo, hi); }
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) { sa.template store<false>(0, u, 0, BK16); sb.template store<false>(0, u, 0, BK16); }
        }
    }
    __syncthreads();
    if (nkt > 1) { sa.load_all(rsA, koff(1) * kstepA); sb.load_all(rsB, koff(1) * kstepB); }
    if (nkt > 0) frags(0, 0);
    for (int t = 0; t < nkt; ++t) {
        const int cur = (t & 1) * STAGE_BYTES, oth = STAGE_BYTES - cur;
        const bool has_next = t + 1 < nkt, stage_last = t + 2 == nkt;
        frags(1, cur);
        mma(0);
        if (has_next) {
            if (stage_last) {
#pragma unroll
                for (int u = 0; u < 4; ++u) sa.template store<true>(oth, u, lo, hi);
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) sa.template store<false>(oth, u, 0, BK16);
            }
        }
        frags(2, cur);
        mma(1);
        if (has_next) {
            if (stage_last) {
#pragma unroll
                for (int u = 0; u < 4; ++u) sb.template store<true>(oth, u, lo, hi);
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) sb.template store<false>(oth, u, 0, BK16);
            }
        }
        frags(3, cur);                                           // every read of this stage is issued before the barrier
        if (has_next) __syncthreads();
        if (t + 2 < nkt) { sa.load_all(rsA, koff(t + 2) * kstepA); sb.load_all(rsB, koff(t + 2) * kstepB); }
        mma(2);
        mma(3);
        if (has_next) frags(0, oth);
    }
    if constexpr (!AKC) {
        if (do_rs) {
            const float r0 = rsum[0] + __shfl_xor(rsum[0], 32, 64);
            const float r1 = rsum[1] + __shfl_xor(rsum[1], 32, 64);
            if (half == 0) {
                float* rs = g.rowsum + bz * g.sRowsum + sp * g.sSplit;
                const int row = m0 + wm * 64 + l31;
                if (row < g.M) rs[row] = r0;
                if (row + 32 < g.M) rs[row + 32] = r1;
            }
        }
    }
    __syncthreads();
    gemm_epilogue(g, acc, tid, m0, n0, bz, sp, wm, wn, half, l31);
}

// The 64.5 KiB of dynamic LDS (two stages; the epilogue image fits inside) keep two workgroups per CU.
int launch_gemm_mfma32(const GemmArgs& g, bool akc, bool bkc, size_t extra_lds, hipStream_t stream) {
    const dim3 grid((unsigned)(g.tiles_m * g.tiles_n), (unsigned)(g.batch * g.splitk)), block(256);
    const size_t lds = LDS_BYTES + extra_lds;
    const hipError_t e = akc && bkc ? launch_dyn_lds<gemm_f32_kernel<true, true>>(grid, block, lds, stream, g)
                         : akc      ? launch_dyn_lds<gemm_f32_kernel<true, false>>(grid, block, lds, stream, g)
                                    : launch_dyn_lds<gemm_f32_kernel<false, false>>(grid, block, lds, stream, g);
    return lds_launch_status(e, "pulse_gemm_f32");
}

int launch_gemm_bf16c(const GemmArgs& g, bool akc, bool bkc, size_t extra_lds, hipStream_t stream) {
    const dim3 grid((unsigned)(g.tiles_m * g.tiles_n), (unsigned)(g.batch * g.splitk)), block(256);
    const size_t lds = LDS_BYTES + extra_lds;
    const hipError_t e = akc && bkc ? launch_dyn_lds<gemm_bf16_kernel<true, true>>(grid, block, lds, stream, g)
                         : akc      ? launch_dyn_lds<gemm_bf16_kernel<true, false>>(grid, block, lds, stream, g)
                                    : launch_dyn_lds<gemm_bf16_kernel<false, false>>(grid, block, lds, stream, g);
    return lds_launch_status(e, "pulse_gemm_f32");
}

}  // namespace pulse
