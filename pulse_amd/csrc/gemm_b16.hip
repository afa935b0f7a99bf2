// The bf16-storage GEMM kernels of the 256-row tiles (pulse_gemm_x3p, planes = 1; gemm_planar.h has what they share with the two-stage kernel of
// gemm_x3p.hip: tile coordinates, LDS images, epilogue).
//
// Three-stage ring ("b16r"): the single-plane form of gemm_x3p_kernel is not limited by the matrix pipe or by power but by the
// latency of its stage DMA (profiles/r04_gemm_b16_pmc.txt: pipe 0.17-0.29 busy at 2.2-2.5 GHz, waves waiting 0.42-0.83 of their cycles):
// with two 72 KB stages only one stage of DMA is ever in flight, issued one stage (1536 SIMD cycles = 0.65 us) before it is needed.
// Same tile (256 x 128, 8 waves of 64 x 64), same fragment / MFMA / epilogue code, but
//   * a stage is 64 k (two 32-deep k-tiles, 48 KB) and THREE stages ring through the same 144 KB: two stages of DMA are in flight while the
//     third is multiplied, and a stage is issued two stages (2048 SIMD cycles) before its first fragment read;
//   * a reduction-contiguous operand is fetched in whole 128-byte lines: one wave instruction = 8 rows x 128 B (both k-tiles of a row),
//     LDS image [row][8 chunks of 16 B], swizzled conflict-free for ds_read_b128
//     (gemm_planar.h, 128-byte image).  (The two-stage kernel fetches 16 rows x 64 B: every line is requested twice, by different instructions.)
//   * [red][out] operands keep the transposing-read image of that kernel, two sub-tiles per stage.
// One barrier per stage, placed before the stage's last k-step: behind it the first fragments of the next stage are read and the DMA of
// stage t + 3 is issued into the buffer stage t has just released.
#include "gemm_planar.h"

namespace pulse {

// Launch LDS of both kernels: 144 KB of stages (the ring's three; the wide kernel's two and the epilogue's transpose image fit inside) and behind
// them the landing strip of the L2 touch loads, 256 B per wave
constexpr int B16_TOUCH_OFF = 144 * 1024, B16_TOUCH_LDS = 256 * 8, B16_LDS = B16_TOUCH_OFF + B16_TOUCH_LDS;
static_assert(256 * XP_CPF * 4 <= B16_TOUCH_OFF, "the epilogue's transpose image fits the launch's LDS");

struct B16rGeom {
    static constexpr int BM = 256, NW = 8, NT = 512, SUBS = 2, NST = 3;
    static constexpr int A_IMG = BM * 64 * SUBS, B_IMG = PBN * 64 * SUBS, STAGE = A_IMG + B_IMG;       // 32 + 16 KB
    static constexpr int A_SUB = BM * 64, B_SUB = PBN * 64;                                         // one 32-deep sub-tile ([red][out] image)
    static constexpr int DMA_PER_WAVE = (STAGE / 1024) / NW;                                        // 6
};
static_assert(3 * B16rGeom::STAGE + B16_TOUCH_LDS <= B16_LDS, "the ring and the touch strip fit the launch's LDS");

template <bool AKC, bool BKC>
__global__ void __launch_bounds__(512) gemm_b16r_kernel(const XpArgs g) {
    using R = B16rGeom;
    extern __shared__ __attribute__((aligned(16))) char xp_smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5, l31 = lane & 31;
    const XpTile T = xp_tile<R::BM, PBN>(g);
    const int nkt32 = T.nkt32;
    const int nst = (nkt32 + 1) / 2;                                 // 64-deep stages

    const int extA = min(R::BM, g.M - T.m0), extB = min(PBN, g.N - T.n0);
    const __amdgpu_buffer_rsrc_t rsA = xp_operand_rsrc<AKC>(g.A + T.bz * g.sA, 0, g.lda, extA, T.klen, T.kpad, T.m0, T.kbeg);
    const __amdgpu_buffer_rsrc_t rsB = xp_operand_rsrc<BKC>(g.B + T.bz * g.sB, 0, g.ldb, extB, T.klen, T.kpad, T.n0, T.kbeg);
    const int voA = AKC ? xp_kc128_lane(lane, wave, g.lda) : xp_ro_lane(lane, g.lda);
    const int voB = BKC ? xp_kc128_lane(lane, wave, g.ldb) : xp_ro_lane(lane, g.ldb);
    const int stA = AKC ? 64 * 2 : 64 * g.lda * 2, stB = BKC ? 64 * 2 : 64 * g.ldb * 2;      // bytes per 64-deep stage
    // unit j of this wave = instruction i = wave + 8 j of the stage's 48 (32 of A, 16 of B)
    auto issue_unit = [&](int stage_off, int t, int j) {
        const int i = wave + j * R::NW;
        if (j * R::NW < 32) {                                        // (j < 4: A; compile-time after unrolling)
            int so, dst;
            if constexpr (AKC) { so = xp_kc128_src(t * stA, i, g.lda); dst = xp_kc128_dst(i); }
            else {
                const int sub = i >> 4, rb = i & 15;                  // sub-tile, row block (8 k groups x 2 out halves of 128)
                so = xp_ro_src(t * stA + sub * 32 * g.lda * 2, rb, g.lda);
                dst = xp_ro_dst(sub, R::A_SUB, rb);
            }
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_t*)(xp_smem + stage_off + dst), 16, voA, so, 0, 0);
        } else {
            const int ib = i - 32;
            int so, dst;
            if constexpr (BKC) { so = xp_kc128_src(t * stB, ib, g.ldb); dst = xp_kc128_dst(ib); }
            else {
                const int sub = ib >> 3, rb = ib & 7;                 // 8 k groups, one out block of 128
                so = xp_ro_src(t * stB + sub * 32 * g.ldb * 2, rb, g.ldb);
                dst = xp_ro_dst(sub, R::B_SUB, rb);
            }
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void_t*)(xp_smem + stage_off + R::A_IMG + dst), 16, voB, so, 0, 0);
        }
    };
    auto issue_stage = [&](int stage_off, int t) {
#pragma unroll
        for (int j = 0; j < R::DMA_PER_WAVE; ++j) issue_unit(stage_off, t, j);
    };
    // L2 touch prefetch of [red][out] operands (see the two-stage kernel): every 128-byte line of stage t is touched two stages before its
    // DMA is issued.  Always issued (past the reduction's end the range check drops them): the barrier waits count them.
    constexpr int LPR_A = R::BM * 2 / 128, LPR_B = PBN * 2 / 128;
    // (only the weight-gradient form, both operands [red][out]: measured, the touches cost the mixed form 4-8 %)
    constexpr int TCH_A = (AKC || BKC) ? 0 : 64 * LPR_A / 64, TCH_B = (AKC || BKC) ? 0 : 64 * LPR_B / 64;
    constexpr int TPW = (TCH_A + TCH_B > 0) ? (TCH_A + TCH_B + R::NW - 1) / R::NW : 0;
    auto touch_stage = [&](int t) {
        if constexpr (TPW > 0) {
#pragma unroll
            for (int j = 0; j < TPW; ++j) {
                const int u = (wave + j * R::NW) % (TCH_A + TCH_B);
                if (u < TCH_A) xp_touch_ro<LPR_A>(rsA, B16_TOUCH_OFF, wave, lane, u, g.lda, t * stA);
                else xp_touch_ro<LPR_B>(rsB, B16_TOUCH_OFF, wave, lane, u - TCH_A, g.ldb, t * stB);
            }
        }
    };

    // fragment read addresses of k-step q4 = 2 kt + ks (kt: 32-deep k-tile of the stage, ks: its 16-deep half), MFMA tile i
    int frA[2][4], frB[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
            const int kt = q4 >> 1, ks = q4 & 1;
            const int oa = wm * 64 + i * 32, ob = wn * 64 + i * 32;         // first row / column of the MFMA tile inside the workgroup's tile
            frA[i][q4] = AKC ? xp_kc128_frag(0, oa + l31, 4 * kt + 2 * ks + half) : xp_ro_frag(kt * R::A_SUB, lane, oa, ks);
            frB[i][q4] = BKC ? xp_kc128_frag(R::A_IMG, ob + l31, 4 * kt + 2 * ks + half) : xp_ro_frag(R::A_IMG + kt * R::B_SUB, lane, ob, ks);
        }

    f32x16 acc[2][2];
    xp_acc_init(g, acc, T.bz, T.n0 + wn * 64 + l31);

    bf16x8 fa[2][2], fb[2][2];                                       // [set][mfma tile]
    auto frag_unit = [&](auto set_tag, int u, int st, int q4) {       // u = 0..3: A0 A1 B0 B1
        constexpr int S = decltype(set_tag)::value;
        if (u < 2) fa[S][u] = xp_frag<AKC>(st + frA[u][q4]);
        else fb[S][u - 2] = xp_frag<BKC>(st + frB[u - 2][q4]);
    };
    // the four MFMAs of a k-step on set S, slot(q) after each
    auto kstep = [&](auto set_tag, bool live, auto&& slot) {
        constexpr int S = decltype(set_tag)::value;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = q >> 1, j = q & 1;
            if (live) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[S][i], fb[S][j], acc[i][j], 0, 0, 0);
            slot(q);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // ---- prologue: stages 0, 1, 2 on their way; stage 0 landed; its first fragments read
    if (nst > 0) issue_stage(0, 0);
    if (nst > 1) issue_stage(R::STAGE, 1);
    if (nst > 2) issue_stage(2 * R::STAGE, 2);
    touch_stage(3);
    touch_stage(4);
    __builtin_amdgcn_sched_barrier(0);
    if (nst > 2) xp_wait_barrier<2 * R::DMA_PER_WAVE + 2 * TPW>();
    else if (nst > 1) xp_wait_barrier<R::DMA_PER_WAVE + 2 * TPW>();
    else xp_wait_barrier<2 * TPW>();
    __builtin_amdgcn_sched_barrier(0);
    if (nst > 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) frag_unit(I0{}, u, 0, 0);
    }

    int cur = 0, nxt = R::STAGE;                                     // byte offsets of the stage being multiplied and of the next one
    for (int t = 0; t < nst; ++t) {
        const bool live1 = 2 * t + 1 < nkt32;                        // the stage's second k-tile exists (wave-uniform)
        kstep(I0{}, true, [&](int q) { frag_unit(I1{}, q, cur, 1); });
        kstep(I1{}, true, [&](int q) { frag_unit(I0{}, q, cur, 2); });
        kstep(I0{}, live1, [&](int q) { frag_unit(I1{}, q, cur, 3); });
        // every fragment read of this stage is issued (lgkmcnt(0) completes them); stage t + 1 has landed (stage t + 2, if it was issued, may
        // still be in flight: it is the youngest DMA of this wave)
        __builtin_amdgcn_sched_barrier(0);
        if (t + 2 < nst) xp_wait_lds_barrier<R::DMA_PER_WAVE + 2 * TPW>();
        else xp_wait_lds_barrier<2 * TPW>();
        __builtin_amdgcn_sched_barrier(0);
        const bool more3 = t + 3 < nst;
        kstep(I1{}, live1, [&](int q) {
            frag_unit(I0{}, q, nxt, 0);                               // (past the last stage: stale bytes nobody multiplies)
            if (more3) { issue_unit(cur, t + 3, q); if (q < R::DMA_PER_WAVE - 4) issue_unit(cur, t + 3, q + 4); }
            if (q == 3) touch_stage(t + 5);
        });
        cur = nxt;
        nxt = nxt + R::STAGE == R::NST * R::STAGE ? 0 : nxt + R::STAGE;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                                // the epilogue reuses the staging buffers
    xp_epilogue<4, 1>(g, acc, tid, wm, wn, half, l31, T.m0, T.n0, T.bz, T.sp, T.tm);
}

// =====================================================================================================================
// bf16-storage GEMM, 256 x 256 tile ("b16w"): the ring kernel stages 384 bytes per MFMA (48 KB per 128 MFMAs of a stage) and is bound
// by the L2 -> LDS path, not by the matrix pipe (profiles/r04_gemm_b16_pmc.txt: pipe 0.24-0.32 busy, no bank conflicts; tools/mfma_feed_probe:
// LDS-DMA sustains 9.6 TB/s from L2 and 6.2-6.7 TB/s from the Infinity Cache / HBM, i.e. 820 / 550 TFLOP/s at 384 B per MFMA).  This kernel
// is the same code on a 256 x 256 output tile: 8 waves of 64 x 128 (eight accumulator tiles, 128 VGPRs), a stage of 64 k = 64 KB for 256
// MFMAs = 256 bytes per MFMA, six fragment reads per eight MFMAs instead of four per four.  Two stages ring through 128 KB: a stage holds twice
// the MFMA work of the ring kernel's, so "issued one stage ahead" is the same 2048 SIMD cycles of lead.  The tile is two 256 x 128 tiles side
// by side (column half p: columns 128 p + 64 wn + 32 j), so images, fragment addresses and the epilogue are the ring kernel's, used twice.
// Used when it does not cost the launch a round of workgroups (xp_wide_tiles, gemm_x3p_api.hip).
struct B16wGeom {
    static constexpr int BM = 256, BN = 256, NW = 8, NT = 512, SUBS = 2, NST = 2;
    static constexpr int A_IMG = BM * 64 * SUBS, B_IMG = BN * 64 * SUBS, STAGE = A_IMG + B_IMG;        // 32 + 32 KB
    static constexpr int A_SUB = BM * 64, B_SUB = BN * 64;
    static constexpr int DMA_PER_WAVE = (STAGE / 1024) / NW;                                        // 8
};
static_assert(2 * B16wGeom::STAGE + B16_TOUCH_LDS <= B16_LDS, "two stages and the touch strip fit the launch's LDS");

template <bool AKC, bool BKC>
__global__ void __launch_bounds__(512) gemm_b16w_kernel(const XpArgs g) {
    using R = B16wGeom;
    extern __shared__ __attribute__((aligned(16))) char xp_smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5, l31 = lane & 31;
    const XpTile T = xp_tile<R::BM, R::BN>(g);
    const int nkt32 = T.nkt32;
    const int nst = (nkt32 + 1) / 2;                                 // 64-deep stages

    const int extA = min(R::BM, g.M - T.m0), extB = min(R::BN, g.N - T.n0);
    const __amdgpu_buffer_rsrc_t rsA = xp_operand_rsrc<AKC>(g.A + T.bz * g.sA, 0, g.lda, extA, T.klen, T.kpad, T.m0, T.kbeg);
    const __amdgpu_buffer_rsrc_t rsB = xp_operand_rsrc<BKC>(g.B + T.bz * g.sB, 0, g.ldb, extB, T.klen, T.kpad, T.n0, T.kbeg);
    // DMA lane offsets and LDS images: the ring kernel's; both operands are 256 rows / columns = 32 instructions per stage each
    const int voA = AKC ? xp_kc128_lane(lane, wave, g.lda) : xp_ro_lane(lane, g.lda);
    const int voB = BKC ? xp_kc128_lane(lane, wave, g.ldb) : xp_ro_lane(lane, g.ldb);
    const int stA = AKC ? 64 * 2 : 64 * g.lda * 2, stB = BKC ? 64 * 2 : 64 * g.ldb * 2;      // bytes per 64-deep stage
    // unit j of this wave = instruction i = wave + 8 j of the stage's 64 (32 of A, 32 of B)
    auto issue_unit = [&](int stage_off, int t, int j) {
        const int i = wave + (j & 3) * R::NW;                        // row block inside the operand
        const int sub = i >> 4, rb = i & 15;                         // [red][out]: sub-tile, (8 k groups x 2 out blocks of 128)
        if (j < 4) {
            int so, dst;
            if constexpr (AKC) { so = xp_kc128_src(t * stA, i, g.lda); dst = xp_kc128_dst(i); }
            else { so = xp_ro_src(t * stA + sub * 32 * g.lda * 2, rb, g.lda); dst = xp_ro_dst(sub, R::A_SUB, rb); }
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_t*)(xp_smem + stage_off + dst), 16, voA, so, 0, 0);
        } else {
            int so, dst;
            if constexpr (BKC) { so = xp_kc128_src(t * stB, i, g.ldb); dst = xp_kc128_dst(i); }
            else { so = xp_ro_src(t * stB + sub * 32 * g.ldb * 2, rb, g.ldb); dst = xp_ro_dst(sub, R::B_SUB, rb); }
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void_t*)(xp_smem + stage_off + R::A_IMG + dst), 16, voB, so, 0, 0);
        }
    };
    // L2 touch prefetch of the weight-gradient form's operands, one stage ahead of the stage's DMA: 4 lines per k row and operand, 64 k rows
    constexpr int LPR = R::BM * 2 / 128;
    constexpr int TCH = (AKC || BKC) ? 0 : 64 * LPR / 64;            // wave instructions per operand and stage
    constexpr int TPW = TCH > 0 ? (2 * TCH + R::NW - 1) / R::NW : 0;
    auto touch_stage = [&](int t) {
        if constexpr (TPW > 0) {
            const int u = wave % (2 * TCH);
            const bool ta = u < TCH;                                  // (wave-uniform)
            xp_touch_ro<LPR>(ta ? rsA : rsB, B16_TOUCH_OFF, wave, lane, u % TCH, ta ? g.lda : g.ldb, t * (ta ? stA : stB));
        }
    };

    // fragment read addresses of k-step q4 = 2 kt + ks: A tile i (rows 64 wm + 32 i), B tile u = 2 p + j (columns 128 p + 64 wn + 32 j)
    int frA[2][4], frB[4][4];
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
        const int kt = q4 >> 1, ks = q4 & 1;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int oa = wm * 64 + i * 32;
            frA[i][q4] = AKC ? xp_kc128_frag(0, oa + l31, 4 * kt + 2 * ks + half) : xp_ro_frag(kt * R::A_SUB, lane, oa, ks);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ob = (u >> 1) * 128 + wn * 64 + (u & 1) * 32;
            frB[u][q4] = BKC ? xp_kc128_frag(R::A_IMG, ob + l31, 4 * kt + 2 * ks + half) : xp_ro_frag(R::A_IMG + kt * R::B_SUB, lane, ob, ks);
        }
    }

    f32x16 acc[2][2][2];                                             // [column half p][i][j]
#pragma unroll
    for (int p = 0; p < 2; ++p) xp_acc_init(g, acc[p], T.bz, T.n0 + p * 128 + wn * 64 + l31);

    bf16x8 fa[2][2], fb[2][4];                                       // [set][tile]
    auto frag_unit = [&](auto set_tag, int u, int st, int q4) {       // u = 0..5: A0 A1 B0 B1 B2 B3
        constexpr int S = decltype(set_tag)::value;
        if (u < 2) fa[S][u] = xp_frag<AKC>(st + frA[u][q4]);
        else if (u < 6) fb[S][u - 2] = xp_frag<BKC>(st + frB[u - 2][q4]);
    };
    // the eight MFMAs of a k-step on set S (A tile outermost: each A fragment feeds four consecutive MFMAs), slot(q) after each
    auto kstep = [&](auto set_tag, bool live, auto&& slot) {
        constexpr int S = decltype(set_tag)::value;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = q >> 2, p = (q >> 1) & 1, j = q & 1;
            if (live) acc[p][i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[S][i], fb[S][2 * p + j], acc[p][i][j], 0, 0, 0);
            slot(q);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto issue_stage = [&](int stage_off, int t) {
#pragma unroll
        for (int j = 0; j < R::DMA_PER_WAVE; ++j) issue_unit(stage_off, t, j);
    };

    long long dbg_w[3] = {0, 0, 0};
    if (g.dbg) dbg_w[0] = wall_clock64();
    // ---- prologue: stages 0 and 1 on their way, the lines of stage 2 touched; stage 0 landed; its first fragments read.
    // vm queue order from here on: [DMA(t + 1) x 8, touch(t + 2)] at the barrier of stage t: vmcnt(TPW) = "DMA(t + 1) has landed".
    if (nst > 0) issue_stage(0, 0);
    if (nst > 1) issue_stage(R::STAGE, 1);
    touch_stage(2);
    __builtin_amdgcn_sched_barrier(0);
    if (nst > 1) xp_wait_barrier<R::DMA_PER_WAVE + TPW>();
    else xp_wait_barrier<TPW>();
    __builtin_amdgcn_sched_barrier(0);
    if (nst > 0) {
#pragma unroll
        for (int u = 0; u < 6; ++u) frag_unit(I0{}, u, 0, 0);
    }

    if (g.dbg) dbg_w[1] = wall_clock64();
    int cur = 0, nxt = R::STAGE;
    for (int t = 0; t < nst; ++t) {
        const bool live1 = 2 * t + 1 < nkt32;                        // the stage's second k-tile exists (wave-uniform)
        kstep(I0{}, true, [&](int q) { frag_unit(I1{}, q, cur, 1); });
        kstep(I1{}, true, [&](int q) { frag_unit(I0{}, q, cur, 2); });
        kstep(I0{}, live1, [&](int q) { frag_unit(I1{}, q, cur, 3); });
        // every fragment read of this stage is issued (lgkmcnt(0) completes them): its buffer is free behind the barrier; stage t + 1 has landed
        __builtin_amdgcn_sched_barrier(0);
        xp_wait_lds_barrier<TPW>();
        __builtin_amdgcn_sched_barrier(0);
        const bool more2 = t + 2 < nst;
        kstep(I1{}, live1, [&](int q) {
            frag_unit(I0{}, q, nxt, 0);                               // (past the last stage: stale bytes nobody multiplies)
            if (more2) issue_unit(cur, t + 2, q);
            if (q == 7) touch_stage(t + 3);
        });
        const int tmp = cur; cur = nxt; nxt = tmp;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                                // the epilogue reuses the staging buffers
    if (g.dbg) dbg_w[2] = wall_clock64();
    xp_epilogue<4, 1>(g, acc[0], tid, wm, wn, half, l31, T.m0, T.n0, T.bz, T.sp, T.tm);
    if (T.n0 + PBN < g.N) {                                         // (workgroup-uniform)
        __syncthreads();
        xp_epilogue<4, 1>(g, acc[1], tid, wm, wn, half, l31, T.m0, T.n0 + PBN, T.bz, T.sp, T.tm);
    }
    if (g.dbg && tid == 0) {                                        // start | first stage landed | main loop done | epilogue's stores issued | all of them acknowledged
        long long* o = g.dbg + 8 * (blockIdx.y * gridDim.x + blockIdx.x);
        o[0] = dbg_w[0]; o[1] = dbg_w[1]; o[2] = dbg_w[2]; o[3] = wall_clock64();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        o[4] = wall_clock64();
        o[5] = (long long)__builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);      // XCC_ID
    }
}

int launch_gemm_b16r(const XpArgs& g, bool akc, bool bkc, hipStream_t stream) {
    const hipError_t e = xp_by_layout(akc, bkc, [&](auto ak, auto bk) {
        return launch_dyn_lds<gemm_b16r_kernel<decltype(ak)::value, decltype(bk)::value>>(xp_grid(g), dim3(512), B16_LDS, stream, g);
    });
    return lds_launch_status(e, "pulse_gemm_x3p");
}
int launch_gemm_b16w(const XpArgs& g, bool akc, bool bkc, hipStream_t stream) {
    const hipError_t e = xp_by_layout(akc, bkc, [&](auto ak, auto bk) {
        return launch_dyn_lds<gemm_b16w_kernel<decltype(ak)::value, decltype(bk)::value>>(xp_grid(g), dim3(512), B16_LDS, stream, g);
    });
    return lds_launch_status(e, "pulse_gemm_x3p");
}

}  // namespace pulse
