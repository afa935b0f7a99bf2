// fp32 GEMM on the bf16 matrix pipe ("x3": three-way operand split, six products).
//
// gfx950's fp32 MFMA (v_mfma_f32_32x32x2_f32) runs at the VALU's rate, 1/16 of the bf16 MFMA.  An fp32 number is the sum of three
// bf16 numbers to within 2^-27 of itself (8 + 8 + 8 significand bits: a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2), round
// to nearest even, the remainders exact; |a2| <= 2^-9 |a|, |a3| <= 2^-18 |a|), every bf16 x bf16 product is exact in fp32, and the
// products that matter at fp32 precision are the six with plane indices i + j <= 2: the dropped ones are below 2^-26 of the product,
// a quarter of an fp32 ulp.  So C = sum_k a b is computed as six v_mfma_f32_32x32x16_bf16 per 16-deep k step, all into the same fp32
// accumulator: fp32-grade results (fewer accumulator roundings per k than the fp32 MFMA's one per 2 k) at up to 16 / 6 = 2.67x the
// fp32 MFMA's matrix-pipe ceiling.  Inputs, outputs and storage are fp32; this is an fp32 GEMM, not a reduced-precision one (tests:
// same fp64-referenced tolerances as the fp32 MFMA kernel; the exactness, linearity and tile-position-independence properties hold bit
// for bit).  Non-finite inputs give NaN (inf - inf in the split).
//
// Tile 128 x 128 x 16, 4 waves, each 2 x 2 MFMA tiles.  LDS image per operand and stage: 3 planes x [2 k-chunks of 8][132 slots][16 B]
// (slot = out ^ ((out >> 3) & 7); a ds_write_b128 is serviced in groups of 8 consecutive lanes over 32 banks, i.e. 4 rows x 2 k-chunks: the chunk stride
// 132 = 4 mod 8 puts the two chunks of a row in different halves of the 128-byte bank window), two stages.  Per thread and k-tile:
// 8 elements of A and 8 of B are split (about 44 VALU each, spread over the first MFMAs of the tile), 6 ds_write_b128, 12
// ds_read_b128 (next tile's fragments, second register set), 24 MFMAs.  Global loads: reduction-contiguous operands 2 x 16 B per
// thread (two lanes per row), [red][out] operands 8 dwords per thread (lane = out: no register transpose).  The buffer resources
// carry the operand's true extent, so loads the hardware range check catches (rows / outs past the operand, k rows past its end) return
// zero without touching memory and no address is clamped.  Correctness does not lean on the check: the k tail is zeroed by a compare in the
// tile that stages the last k-tile, and rows / outs beyond the extent only feed outputs that are never stored.
#include <type_traits>
#include "common.h"
#include "gemm_shared.h"
#include "gemm_epilogue.h"

namespace pulse {

#ifndef X3_CSTRIDE
#define X3_CSTRIDE 132
#endif
constexpr int X_CSTRIDE = X3_CSTRIDE;               // 16-byte slots per 8-k chunk block (see the store-pattern note above)
constexpr int X_PLANE = 2 * X_CSTRIDE * 16;          // 4,224 B
constexpr int X_IMG = 3 * X_PLANE;                   // 12,672 B per operand
constexpr int X_STAGE = 2 * X_IMG;                   // 25,344 B
#ifndef X3_BARRIER_GAP
#define X3_BARRIER_GAP 13
#endif
constexpr int X_LDS = BM * CP * 4;                   // 65,536 B: the epilogue transpose (>= 2 stages = 50,688 B) -> two workgroups per CU

template <bool KC>
struct StagerX {
    float v[2][8];       // two register sets (tile parity): loads run two tiles ahead of their split.  KC: two 16-byte loads; MC: 8 dwords
    int voff;            // per-lane byte offset (constant); the k advance and MC's row advance are scalar offsets
    int lds;
    int kpos;
    int ld4;             // MC: bytes per k row (wave-uniform)

    __device__ __forceinline__ void init(int tid, int ld, int img_off) {
        ld4 = ld * 4;
        if constexpr (KC) {
            const int row = tid >> 1, kc = tid & 1;
            kpos = kc * 8;
            voff = (row * ld + kc * 8) * 4;
            lds = img_off + (kc * X_CSTRIDE + slot_of(row)) * 16;
        } else {
            const int out = tid & 127, kch = tid >> 7;
            kpos = kch * 8;
            voff = (kch * 8 * ld + out) * 4;
            lds = img_off + (kch * X_CSTRIDE + slot_of(out)) * 16;
        }
    }
    template <int S>
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rs, int soff) {
        if constexpr (KC) {
            const f32x4 a = buf_load(rs, voff, soff), b = buf_load(rs, voff, soff + 16);
            v[S][0] = a.x; v[S][1] = a.y; v[S][2] = a.z; v[S][3] = a.w; v[S][4] = b.x; v[S][5] = b.y; v[S][6] = b.z; v[S][7] = b.w;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[S][i] = bitsf(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff + i * ld4, 0));
        }
    }
    template <int S, bool MASKED>
    __device__ __forceinline__ void mask(int hi) {
        if constexpr (MASKED) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (kpos + e >= hi) v[S][e] = 0.f;
        }
    }
    template <int S>
    __device__ __forceinline__ float sum8() const {
        return ((v[S][0] + v[S][1]) + (v[S][2] + v[S][3])) + ((v[S][4] + v[S][5]) + (v[S][6] + v[S][7]));
    }
    // split element pair k (elements 2k, 2k+1) into the three planes' packed dwords: round-to-nearest-even at every level
    // (v_cvt_pk_bf16_f32), remainders exact (the difference of a float and its 8-bit rounding is representable)
    u32x4 p0, p1, p2;
    template <int S>
    __device__ __forceinline__ void split_pair(int k) {
        const float a = v[S][2 * k], b = v[S][2 * k + 1];
        const unsigned q0 = pack_rn(a, b);
        p0[k] = q0;
        const float ra = a - bitsf(q0 << 16), rb = b - bitsf(q0 & 0xffff0000u);
        const unsigned q1 = pack_rn(ra, rb);
        p1[k] = q1;
        const float sa = ra - bitsf(q1 << 16), sb = rb - bitsf(q1 & 0xffff0000u);
        p2[k] = pack_rn(sa, sb);
    }
    __device__ __forceinline__ void write_plane(int st, int pl) {
        extern __shared__ __attribute__((aligned(16))) char smem_c[];
        *reinterpret_cast<u32x4*>(smem_c + st + lds + pl * X_PLANE) = pl == 0 ? p0 : pl == 1 ? p1 : p2;
    }
    __device__ __forceinline__ void write(int st) { write_plane(st, 0); write_plane(st, 1); write_plane(st, 2); }
};

// WM = 32-row MFMA tiles per wave: 2 = the 128-row tile, 1 = a 64-row tile (half the MFMAs per k-tile beside the same B staging) for
// skinny launches whose 128-row tiling would leave the chip at one workgroup per CU (the mu / value heads).
template <bool AKC, bool BKC, int WM>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) gemm_x3_kernel(const GemmArgs g) {
    constexpr int BMx = 64 * WM;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int half = lane >> 5;
    const int l31 = lane & 31;
    const WgMap wg = map_workgroup(g.tiles_m * g.tiles_n, g.batch, g.splitk);
    const int id = wg.id;
    const int tm = id / g.tiles_n, tn = id - tm * g.tiles_n;
    const int m0 = tm * BMx, n0 = tn * BN;
    const int bz = wg.bz, sp = wg.sp;
    const int kbeg = sp * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const int klen = kend - kbeg;
    const int nkt = (klen + XK - 1) / XK;
    const int hi = klen - (nkt - 1) * XK;                       // valid k positions of the last tile (1 .. 16)

    long long dbg_c0 = 0, dbg_w0 = 0, dbg_c1 = 0, dbg_w1 = 0;
    if (g.dbg) { dbg_c0 = clock64(); dbg_w0 = wall_clock64(); }

    // buffer resources with the TRUE extent from this workgroup's origin: what the range check catches reads as zero (no memory access)
    const int extA = min(BMx, g.M - m0), extB = min(BN, g.N - n0);
    const int k4rem = ((g.K + 3) & ~3) - kbeg;                   // readable k positions of a reduction-contiguous row from kbeg
    const float* Ab = g.A + bz * g.sA + (AKC ? (long long)m0 * g.lda + kbeg : (long long)kbeg * g.lda + m0);
    const float* Bb = g.B + bz * g.sB + (BKC ? (long long)n0 * g.ldb + kbeg : (long long)kbeg * g.ldb + n0);
    const unsigned recA = (unsigned)(AKC ? ((extA - 1) * g.lda + k4rem) : ((klen - 1) * g.lda + extA)) * 4u;
    const unsigned recB = (unsigned)(BKC ? ((extB - 1) * g.ldb + k4rem) : ((klen - 1) * g.ldb + extB)) * 4u;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Ab), 0, klen > 0 ? recA : 0u, RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Bb), 0, klen > 0 ? recB : 0u, RSRC_FLAGS);
    const int kstepA = (AKC ? 4 : g.lda * 4) * XK, kstepB = (BKC ? 4 : g.ldb * 4) * XK;      // bytes per k-tile

    StagerX<AKC> sa;
    StagerX<BKC> sb;
    sa.init(tid, g.lda, 0);
    sb.init(tid, g.ldb, X_IMG);

    // fragment read addresses: lane (l31, half) reads out (wm|wn) * 64 + {0, 32} + l31, k-chunk = half, plane p at + p * X_PLANE
    const int frA0 = (half * X_CSTRIDE + slot_of(wm * 32 * WM + l31)) * 16;
    const int frA1 = (half * X_CSTRIDE + slot_of(wm * 32 * WM + 32 + l31)) * 16;      // WM == 2 only
    const int frB0 = X_IMG + (half * X_CSTRIDE + slot_of(wn * 64 + l31)) * 16;
    const int frB1 = X_IMG + (half * X_CSTRIDE + slot_of(wn * 64 + 32 + l31)) * 16;

    f32x16 acc[WM][2];
    {
        float b0 = 0.f, b1 = 0.f;
        if (g.epi == 0 && g.bias) {
            const float* bias = g.bias + bz * g.sBias;
            const int c0 = n0 + wn * 64 + l31;
            if (c0 < g.N) b0 = bias[c0];
            if (c0 + 32 < g.N) b1 = bias[c0 + 32];
        }
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][0][r] = b0; acc[i][1][r] = b1; }
    }
    float rs_acc = 0.f;
    const bool do_rs = !AKC && g.rowsum != nullptr && tn == 0;      // workgroup-uniform: the stager of A sums its k rows (bias gradient)

    // Fragment registers: plane 0 in two sets (tile parity), planes 1 and 2 in ONE set that is refilled as soon as the tile's last
    // MFMA reading it has issued.  Term order (A plane, B plane): (2,0) (0,2) (1,1) (1,0) (0,1) (0,0)  =>  A2 is dead after MFMA 3,
    // B2 after 7, A1 after 15, B1 after 19.
    bf16x8 fa0[2][WM], fb0[2][2], fa1[WM], fb1[2], fa2[WM], fb2[2];
    // fragment read unit u (0..11) of the stage at byte offset st (plane 0 into set S), in the order the slots allow
    auto frag_unit = [&](auto set_tag, int u, int st) {
        constexpr int S = decltype(set_tag)::value;
        extern __shared__ __attribute__((aligned(16))) char smem_c[];
        auto rd = [&](int addr) { return *reinterpret_cast<const bf16x8*>(smem_c + st + addr); };
        switch (u) {
            case 0: fa2[0] = rd(frA0 + 2 * X_PLANE); break;
            case 1: if constexpr (WM == 2) fa2[1] = rd(frA1 + 2 * X_PLANE); break;
            case 2: fb0[S][0] = rd(frB0); break;
            case 3: fb0[S][1] = rd(frB1); break;
            case 4: fb2[0] = rd(frB0 + 2 * X_PLANE); break;
            case 5: fb2[1] = rd(frB1 + 2 * X_PLANE); break;
            case 6: fa0[S][0] = rd(frA0); break;
            case 7: if constexpr (WM == 2) fa0[S][1] = rd(frA1); break;
            case 8: fa1[0] = rd(frA0 + X_PLANE); break;
            case 9: if constexpr (WM == 2) fa1[1] = rd(frA1 + X_PLANE); break;
            case 10: fb1[0] = rd(frB0 + X_PLANE); break;
            default: fb1[1] = rd(frB1 + X_PLANE); break;
        }
    };

    // One k-tile = 24 MFMAs (6 plane pairs x 4 accumulator tiles; an accumulator is reused every 4th MFMA), one unit of side work
    // after each:
    //   slots 0-7    split of tile t+1: A pairs 0-3, B pairs 0-3 (its loads were issued TWO tiles ago: a tile is only ~770 MFMA
    //                cycles per wave, far less than the memory latency)
    //   slots 4-6, 8-10   A's / B's three ds_write_b128, one per slot
    //   slot 11      global loads of tile t+3 into the register set tile t+1 just left
    //   slot 13      the ONE barrier of the tile (its lgkmcnt wait falls three MFMAs after the last store)
    //   slots 14-17  next tile's fragment reads A2 B0' B2 A0' (two per slot), slot 20: A1 (dead after MFMA 15), slot 22: B1 (after 19)
    // MODE 0 steady, 1 = stages the LAST tile (k tail zeroed, no further loads), 2 = last tile (compute only).
    auto tile = [&](auto mode_tag, auto stage_tag, int t) {
        constexpr int MODE = decltype(mode_tag)::value;
        constexpr int S = decltype(stage_tag)::value;
        constexpr int OTH = (1 - S) * X_STAGE;
        using SetO = std::integral_constant<int, 1 - S>;
        constexpr int O = 1 - S;                                  // register set / stage of tile t+1 (and t+3)
        if constexpr (MODE != 2) {
            sa.template mask<O, MODE == 1>(hi);
            sb.template mask<O, MODE == 1>(hi);
            if constexpr (!AKC) {
                if (do_rs) rs_acc += sa.template sum8<O>();
            }
        }
        // the side-work schedule is written in 24 SLOTS (slot s belongs to term s / 4); with WM == 2 every slot follows its own MFMA,
        // with WM == 1 the tile has 12 MFMAs and each is followed by two slots
        constexpr int SPM = 2 / WM;
#pragma unroll
        for (int q = 0; q < 12 * WM; ++q) {
            {
                const int term = q / (2 * WM), i = (q >> 1) % WM, j = q & 1;
                const bf16x8 a = term == 0 ? fa2[i] : (term == 2 || term == 3) ? fa1[i] : fa0[S][i];
                const bf16x8 b = term == 1 ? fb2[j] : (term == 2 || term == 4) ? fb1[j] : fb0[S][j];
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[i][j], 0, 0, 0);
            }
#pragma unroll
            for (int p = q * SPM; p < (q + 1) * SPM; ++p)
            if constexpr (MODE != 2) {
                if (p < 4) sa.template split_pair<O>(p);
                else if (p < 8) sb.template split_pair<O>(p - 4);
                if (p >= 4 && p < 7) sa.write_plane(OTH, p - 4);          // one 16-byte store per gap: the store path takes ~13 cycles each
                if (p >= 8 && p < 11) sb.write_plane(OTH, p - 8);
                if constexpr (MODE == 0) {
                    if (p == 11 && t + 3 < nkt) {
                        sa.template load<O>(rsA, (t + 3) * kstepA); sb.template load<O>(rsB, (t + 3) * kstepB);
                    }
                }
                if (p == X3_BARRIER_GAP) {                                // a few MFMAs after the last store: its lgkmcnt wait is short
                    __builtin_amdgcn_sched_barrier(0);
                    __syncthreads();
                }
                {
                    // 12 fragment reads in the gaps after the barrier; A1 may be refilled after MFMA 15, B1 after MFMA 19
                    constexpr int R0 = X3_BARRIER_GAP + 1;
                    if (p == R0) { frag_unit(SetO{}, 0, OTH); frag_unit(SetO{}, 1, OTH); }
                    else if (p == R0 + 1) { frag_unit(SetO{}, 2, OTH); frag_unit(SetO{}, 3, OTH); }
                    else if (p == R0 + 2) { frag_unit(SetO{}, 4, OTH); frag_unit(SetO{}, 5, OTH); }
                    else if (p == R0 + 3) { frag_unit(SetO{}, 6, OTH); frag_unit(SetO{}, 7, OTH); }
                    if (p == 20) { frag_unit(SetO{}, 8, OTH); frag_unit(SetO{}, 9, OTH); }
                    if (p == 22) { frag_unit(SetO{}, 10, OTH); frag_unit(SetO{}, 11, OTH); }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>; using I2 = std::integral_constant<int, 2>;

    if (nkt > 0) {
        sa.template load<0>(rsA, 0); sb.template load<0>(rsB, 0);
        if (nkt > 1) { sa.template load<1>(rsA, kstepA); sb.template load<1>(rsB, kstepB); }
        if (nkt == 1) { sa.template mask<0, true>(hi); sb.template mask<0, true>(hi); }
        if constexpr (!AKC) {
            if (do_rs) rs_acc += sa.template sum8<0>();
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { sa.template split_pair<0>(k); sb.template split_pair<0>(k); }
        sa.write(0); sb.write(0);
    }
    __syncthreads();
    if (nkt > 2) { sa.template load<0>(rsA, 2 * kstepA); sb.template load<0>(rsB, 2 * kstepB); }
    if (nkt > 0) {
#pragma unroll
        for (int u = 0; u < 12; ++u) frag_unit(I0{}, u, 0);
    }
    {
        int t = 0;
        for (; t + 3 < nkt; t += 2) { tile(I0{}, I0{}, t); tile(I0{}, I1{}, t + 1); }
        if (t + 2 < nkt) {
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
    __syncthreads();                                              // the epilogue (and the row-sum exchange) reuse the staging buffers
    if constexpr (!AKC) {
        if (do_rs) {
            extern __shared__ __attribute__((aligned(16))) float smem[];
            smem[tid] = rs_acc;                                   // thread (kch = tid >> 7, out = tid & 127) summed its 8 k rows of every tile
            __syncthreads();
            if (tid < BMx && m0 + tid < g.M) g.rowsum[bz * g.sRowsum + sp * g.sSplit + m0 + tid] = smem[tid] + smem[tid + 128];
            __syncthreads();
        }
    }
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

// ``half_tile``: the 64-row tile (``g.tiles_m`` counts 64-row tiles then)
int launch_gemm_x3(const GemmArgs& g, bool akc, bool bkc, bool half_tile, size_t extra_lds, hipStream_t stream) {
    const dim3 grid((unsigned)(g.tiles_m * g.tiles_n), (unsigned)(g.batch * g.splitk)), block(256);
    const size_t lds = X_LDS + extra_lds;
    hipError_t e;
    if (half_tile)
        e = akc && bkc ? launch_dyn_lds<gemm_x3_kernel<true, true, 1>>(grid, block, lds, stream, g)
            : akc      ? launch_dyn_lds<gemm_x3_kernel<true, false, 1>>(grid, block, lds, stream, g)
                       : launch_dyn_lds<gemm_x3_kernel<false, false, 1>>(grid, block, lds, stream, g);
    else
        e = akc && bkc ? launch_dyn_lds<gemm_x3_kernel<true, true, 2>>(grid, block, lds, stream, g)
            : akc      ? launch_dyn_lds<gemm_x3_kernel<true, false, 2>>(grid, block, lds, stream, g)
                       : launch_dyn_lds<gemm_x3_kernel<false, false, 2>>(grid, block, lds, stream, g);
    return lds_launch_status(e, "pulse_gemm_f32");
}

}  // namespace pulse
