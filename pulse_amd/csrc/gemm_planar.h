// Pieces shared by the planar GEMM translation units (gemm_x3p.hip: the two-stage kernel, three planes or one; gemm_b16.hip: the bf16-storage ring and
// 256 x 256 kernels; gemm_x3p_api.hip: pulse_gemm_x3p, which chooses between them): the launch argument block, the LDS read helpers, the tile front
// end -- tile coordinates, operand buffer resources, the LDS images' address formulas (DMA side and fragment side of an image live HERE ONLY, next
// to each other: they must agree), bias-initialised accumulators, the touch load -- and the epilogue.  What is measured stays in the kernels: geometry,
// the main-loop schedule, the vmcnt counts and barrier placement, the prologue.
#pragma once
#include <type_traits>
#include "gemm_shared.h"

namespace pulse {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_t;

constexpr int PK = 32;                 // k per tile
constexpr int PBN = 128;               // tile columns
constexpr int ROWB = PK * 2;           // bytes of one plane row of a reduction-contiguous tile
constexpr unsigned P_RSRC = 0x00020000u;
constexpr int XP_CPF = PBN + 4;        // epilogue transpose pitch (floats)

struct XpArgs {
    const unsigned short* A; const unsigned short* B;
    long long pa, pb;                  // plane strides (elements)
    int lda, ldb;                      // pitches (elements)
    float* C; float* C2; unsigned short* Cp; const float* bias; const float* aux; const unsigned short* aux16;
    long long pc;                      // plane stride of Cp (elements)
    int ldc, ldc2, ldcp, ldaux;
    int M, N, K;
    long long sA, sB, sC, sC2, sCp, sBias, sAux;   // batch strides (elements of the respective arrays)
    int batch, splitk, kchunk;
    long long sSplit;
    int act, epi;
    int tiles_m, tiles_n;
    float* rowsum; long long sRowsum;
    float* colsum; long long sColsum; int ldcs;      // optional: per-row-tile column sums of the OUTPUT (colsum[bz * sColsum + tm * ldcs + n])
    long long* dbg;                                  // optional per-workgroup wall-clock stamps (tools/gemm_b16_phases.py; pulse_gemm_set_debug_buffer)
    unsigned char* mask8; int ldm8; long long sM8;   // ReLU bit mask, one byte per (row, 8 columns): written by EPI 0 + relu, read by EPI 1 when there is no aux
    int general_rows;                                // gemm option 9 (tests): every epilogue row through the general form
};

// ---- LDS reads ------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bf16x8 xp_lds128(int addr) {
    extern __shared__ __attribute__((aligned(16))) char xp_smem[];
    return *reinterpret_cast<const bf16x8*>(xp_smem + addr);
}
// [red][out] fragment: 8 consecutive k of one out = two transposing 8-byte reads (k rows 0-3 and 4-7 of the lane's k-chunk)
__device__ __forceinline__ bf16x8 xp_lds_tr(int addr_lo, int addr_hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char xp_smem[];
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(xp_smem + addr_lo));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(xp_smem + addr_hi));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 v = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return __builtin_bit_cast(bf16x8, v);
#else
    // host pass of the single-source compile: the gfx950-only builtin does not exist there, and a kernel template whose instantiation
    // reaches it is silently not emitted (its launch stub goes missing at link time)
    return bf16x8{};
#endif
}
// the fragment at ``addr`` of an operand image.  KC: the operand is stored [out][k] (reduction-contiguous); otherwise [k][out] ("[red][out]")
template <bool KC>
__device__ __forceinline__ bf16x8 xp_frag(int addr) {
    if constexpr (KC) return xp_lds128(addr);
    else return xp_lds_tr(addr, addr + 1024);
}
using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;      // fragment set / stage tags of the kernels' lambdas

// ---- tile coordinates -----------------------------------------------------------------------------------------------------------------------------
// XCD-aware remap (common.h map_workgroup; block b runs on XCD b % 8): every XCD owns a contiguous band of output tiles, or -- split-K
// launches, i.e. the weight gradients -- a K RANGE of both operands, so an operand element crosses the fabric once instead of once per XCD
struct XpTile {
    int tm, tn, m0, n0, bz, sp;        // tile indices, its first row / column, batch slot, k split
    int kbeg, klen, nkt32, kpad;       // this split's k range, its 32-deep k-tiles, klen rounded up to them (the planes are zero-padded to a multiple of 32 in k)
};
template <int BM, int BN>
__device__ __forceinline__ XpTile xp_tile(const XpArgs& g) {
    const WgMap wgm = map_workgroup(g.tiles_m * g.tiles_n, g.batch, g.splitk);
    XpTile t;
    t.tm = wgm.id / g.tiles_n; t.tn = wgm.id - t.tm * g.tiles_n;
    t.m0 = t.tm * BM; t.n0 = t.tn * BN;
    t.bz = wgm.bz; t.sp = wgm.sp;
    t.kbeg = t.sp * g.kchunk;
    t.klen = min(g.K, t.kbeg + g.kchunk) - t.kbeg;
    t.nkt32 = (t.klen + PK - 1) / PK;
    t.kpad = t.nkt32 * PK;
    return t;
}

// ---- buffer resource of one operand plane, based at this workgroup's tile origin (first out ``out0``, first k ``kbeg``), with the true extent
// ``ext`` outs x ``klen`` k: rows / outs past the operand read as zero and write zeros into LDS; they only feed outputs that are never stored.
// ``base``: the batch slot's matrix, ``plane``: the plane's offset from it (elements).  (``ext`` must not be template-dependent at the call: that
// makes the host pass drop the kernel's stub.)
template <bool KC>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t xp_operand_rsrc(const unsigned short* base, long long plane, int ld, int ext, int klen, int kpad,
                                                                  int out0, int kbeg) {
    const unsigned short* p = base + plane + (KC ? (long long)out0 * ld + kbeg : (long long)kbeg * ld + out0);
    const unsigned r = (unsigned)(KC ? ((ext - 1) * ld + kpad) : ((klen - 1) * ld + ((ext + 7) & ~7))) * 2u;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(p), 0, klen > 0 ? r : 0u, P_RSRC);
}

// ==== LDS images.  One DMA wave instruction fills 1024 consecutive LDS bytes (lane L: bytes 16 L ..), which fixes every image to be lane-linear
// per instruction; the swizzle is applied to the SOURCE address.  Per image: the lane's DMA source offset (bytes, constant; the k-tile / stage
// advance is the caller's scalar offset), an instruction's ("unit's") source offset and LDS destination, and the fragment read address
// (``base``: what the caller adds -- the k-tile's / stage's source offset, the image's place in the stage).

// ---- [red][out] image of a 32-deep sub-tile (all three kernels, A and B): [128-out block][32 k rows][16 pieces of 16 B], piece p of k row m at
// slot p ^ ((m & 3) << 2): the four rows x four pieces a half-wave's transposing read touches are 16 different bank groups.
// Row block rb of a sub-tile = one instruction: 4 k rows x 16 pieces of one 128-out block: block rb >> 3, k rows 4 (rb & 7) + (L >> 4), slot L & 15
// holding piece (L & 15) ^ ((L >> 4) << 2).
__device__ __forceinline__ int xp_ro_lane(int lane, int ld) { return ((lane >> 4) * ld + (((lane & 15) ^ ((lane >> 4) << 2)) << 3)) * 2; }
__device__ __forceinline__ int xp_ro_src(int base, int rb, int ld) { return base + (rb & 7) * 4 * ld * 2 + (rb >> 3) * 256; }
__device__ __forceinline__ int xp_ro_dst(int sub, int sub_stride, int rb) { return sub * sub_stride + rb * 1024; }
// Fragment of k-step ks (16-deep half of the sub-tile) for the 32-out MFMA tile that starts at out ``o`` (block o >> 7, out o & 127): 16-lane group
// gq = lane >> 4 covers outs 16 (gq & 1) .. + 15 of the tile and k rows 8 (gq >> 1) .. + 7 of the k-step; lane 4 j + q of the group addresses k row j
// (second read: j + 4, + 1024 bytes), 8-byte piece q of those 16 outs, and receives the four k values of out (lane & 15) (ds_read_b64_tr_b16;
// tools/tr_probe.cpp)
__device__ __forceinline__ int xp_ro_frag(int base, int lane, int o, int ks) {
    const int gq = lane >> 4, jj = (lane >> 2) & 3, qq = lane & 3;
    const int og = o + 16 * (gq & 1);                               // first out of this group
    const int piece = ((og & 127) >> 3) + (qq >> 1);
    return base + ks * 4096 + (og >> 7) * 8192 + (8 * (gq >> 1) + jj) * 256 + ((piece ^ (jj << 2)) << 4) + (qq & 1) * 8;
}

// ---- 64-byte reduction-contiguous image (two-stage kernel), per plane: [row][4 slots of 16 B] = [row][32 k], slot s of row r holding k-chunk
// s ^ ((r >> 2) & 3): the fragment reads (32 consecutive rows, one chunk) hit every bank once.
// Row block rb = one instruction: 16 rows x 4 chunks: lane L -> row 16 rb + (L >> 2), slot L & 3 holding chunk (L & 3) ^ ((L >> 4) & 3).
__device__ __forceinline__ int xp_kc64_lane(int lane, int ld) { return ((lane >> 2) * ld + (((lane & 3) ^ ((lane >> 4) & 3)) << 3)) * 2; }
__device__ __forceinline__ int xp_kc64_src(int base, int rb, int ld) { return base + rb * 16 * ld * 2; }
__device__ __forceinline__ int xp_kc64_dst(int rb) { return rb * 1024; }
// lane (l31, half) of k-step ks reads chunk 2 ks + half of its row
__device__ __forceinline__ int xp_kc64_frag(int base, int row, int chunk) { return base + (row * 4 + (chunk ^ ((row >> 2) & 3))) * 16; }

// ---- 128-byte reduction-contiguous image (ring and wide kernels): [row][8 chunks of 16 B] = [row][64 k], whole 128-byte lines.
// Row block i = one instruction: 8 rows x 128 B: lane L -> row 8 i + (L >> 3), LDS slot L & 7 holding chunk (L & 7) ^ ((r >> 1) & 7).
// Swizzle: chunk c of row r sits at slot c ^ ((r >> 1) & 7).  ds_read_b128 is serviced in four 16-lane groups ({0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} and the same + 32: MI355X_MICROARCH.md, LDS table) over a 256-byte bank row = two 128-byte tile rows: the eight even
// and the eight odd rows of every group then carry eight different values of (r >> 1) & 7 -- conflict-free.  (c ^ (r & 7), the first
// version, put rows 12 and 20 of a group on the same slot: SQ_LDS_BANK_CONFLICT was half of SQ_LDS_IDX_ACTIVE.)  Row 8 i + (L >> 3) of
// instruction i: (r >> 1) & 7 = (4 i + (L >> 4)) & 7, and i has the wave's parity (instruction i = wave + 8 j of an 8-wave workgroup).
__device__ __forceinline__ int xp_kc128_lane(int lane, int wave, int ld) {
    const int kcx = (4 * (wave & 1) + (lane >> 4)) & 7;
    return ((lane >> 3) * ld + (((lane & 7) ^ kcx) << 3)) * 2;
}
__device__ __forceinline__ int xp_kc128_src(int base, int i, int ld) { return base + i * 8 * ld * 2; }
__device__ __forceinline__ int xp_kc128_dst(int i) { return i * 1024; }
__device__ __forceinline__ int xp_kc128_frag(int base, int row, int chunk) { return base + row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

// ---- the 2 x 2 accumulator block of one 128-column half, initialised with the bias (EPI 0): c0 = this lane's first column (n0 + 64 wn + l31)
__device__ __forceinline__ void xp_acc_init(const XpArgs& g, f32x16 (&acc)[2][2], int bz, int c0) {
    float b0 = 0.f, b1 = 0.f;
    if (g.epi == 0 && g.bias) {
        const float* bias = g.bias + bz * g.sBias;
        if (c0 < g.N) b0 = bias[c0];
        if (c0 + 32 < g.N) b1 = bias[c0 + 32];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[i][0][r] = b0; acc[i][1][r] = b1; }
}

// ---- L2 touch: gfx950 has no prefetch instruction, so a 128-byte line is touched by a 4-byte LDS-DMA load into the wave's 256 bytes of a scratch
// strip at ``touch_off`` (no VGPR destination, no register hazard): the line is in L2 when the real DMA asks for it.  One wave instruction touches
// 64 lines: lines 64 u .. 64 u + 63 of a [red][out] operand's stage, LPR lines per k row.  Past the reduction's end the range check drops it.
template <int LPR>
__device__ __forceinline__ void xp_touch_ro(__amdgpu_buffer_rsrc_t rs, int touch_off, int wave, int lane, int u, int ld, int so) {
    extern __shared__ __attribute__((aligned(16))) char xp_smem[];
    const int q = 64 * u + lane;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(xp_smem + touch_off + wave * 256), 4, (q / LPR) * ld * 2 + (q % LPR) * 128, so, 0, 0);
}

// ---- "all but the youngest N vector-memory operations of this wave have landed" + workgroup barrier; the form inside the main loop also completes
// the wave's LDS reads.  The counts and where the barriers stand are each kernel's own.
template <int N> __device__ __forceinline__ void xp_wait_barrier() { asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void xp_wait_lds_barrier() { asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory"); }

// ---- epilogue of the planar kernels (WMW x 2 waves of 64 x 64 on a 64 WMW x 128 tile): accumulators -> LDS (fp32, pitch CPF) -> rows of 8 consecutive columns per lane -> fp32 C and / or
// the output's own planes (bf16 matrix in single-plane mode), optional per-row-tile column sums.  The caller has drained its DMA and passed a
// barrier: the staging buffers are free.
template <int WMW, int NPL>
__device__ __forceinline__ void xp_epilogue(const XpArgs& g, f32x16 (&acc)[2][2], int tid, int wm, int wn, int half, int l31, int m0, int n0, int bz,
                                            int sp, int tm) {
    constexpr int BM = 64 * WMW, NT = 128 * WMW;                    // tile rows, threads (WMW: waves along M; two along N)
    extern __shared__ __attribute__((aligned(16))) char xp_smem[];
    float* sC = reinterpret_cast<float*>(xp_smem);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                sC[(wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * XP_CPF + wn * 64 + j * 32 + l31] = acc[i][j][r];
    __syncthreads();
    if (g.dbg && tid == 0) g.dbg[8 * (blockIdx.y * gridDim.x + blockIdx.x) + 6] = wall_clock64();     // (diagnostics: transpose image written)
    {
        float* C = g.C ? g.C + bz * g.sC + sp * g.sSplit : nullptr;
        float* C2 = g.C2 ? g.C2 + bz * g.sC2 : nullptr;
        unsigned short* Cp = g.Cp ? g.Cp + bz * g.sCp : nullptr;
        const float* aux = g.aux ? g.aux + bz * g.sAux : nullptr;
        const unsigned short* aux16 = g.aux16 ? g.aux16 + bz * g.sAux : nullptr;
        unsigned char* mask8 = g.mask8 ? g.mask8 + bz * g.sM8 : nullptr;
        const bool use_mask = g.epi == 1 && aux == nullptr && aux16 == nullptr;
        const int c8 = (tid & 15) * 8;
        const int col = n0 + c8;
        constexpr int RPI = NT / 16;                             // rows per iteration
        float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // column sums of what this thread stores (the bias gradient of the producer layer)
        if (col < g.N) {
            const bool full = col + 7 < g.N;
            // one row of 8 columns: image -> rounding / activation / mask -> C, Cp, column sums
            auto do_row = [&](int rl, const f32x4 v0, const f32x4 v1) {
                const int row = m0 + rl;
                float o[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                if constexpr (NPL == 1) {
                    // a bf16 autocast Linear hands bf16 to the next op: the product leaves rounded, the activation / mask acts on that
                    // (split-K slabs are partial sums and stay fp32)
                    if (g.splitk == 1) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) o[k] = rbf(o[k]);
                    }
                }
                if (g.epi == 0) {
                    if (g.act == 1) {
                        if (mask8) {                                // the sign bits of this thread's eight outputs: one byte nobody else touches
                            unsigned bits = 0;
#pragma unroll
                            for (int k = 0; k < 8; ++k) bits |= (col + k < g.N && o[k] > 0.f ? 1u : 0u) << k;
                            mask8[(long long)row * g.ldm8 + (col >> 3)] = (unsigned char)bits;
                        }
#pragma unroll
                        for (int k = 0; k < 8; ++k) o[k] = fmaxf(o[k], 0.f);
                    } else if (g.act == 2) {
                        if (C2) {
                            float* p2 = C2 + (long long)row * g.ldc2 + col;
                            if (full) { *reinterpret_cast<f32x4*>(p2) = (f32x4){o[0], o[1], o[2], o[3]}; *reinterpret_cast<f32x4*>(p2 + 4) = (f32x4){o[4], o[5], o[6], o[7]}; }
                            else for (int k = 0; k < 8 && col + k < g.N; ++k) p2[k] = o[k];
                        }
#pragma unroll
                        for (int k = 0; k < 8; ++k) o[k] = silu(o[k]);
                    }
                } else if (use_mask) {                              // relu-grad from the forward's sign bits (one byte instead of 16 / 32 of activations)
                    const unsigned bits = mask8[(long long)row * g.ldm8 + (col >> 3)];
#pragma unroll
                    for (int k = 0; k < 8; ++k) o[k] = ((bits >> k) & 1u) ? o[k] : 0.f;
                } else {
                    float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    if (aux16) {                                    // bf16-stored activations (rows hold roundup8(N) columns)
                        const u32x4 t = *reinterpret_cast<const u32x4*>(aux16 + (long long)row * g.ldaux + col);
#pragma unroll
                        for (int k = 0; k < 4; ++k) { a8[2 * k] = split_bitsf(t[k] << 16); a8[2 * k + 1] = split_bitsf(t[k] & 0xffff0000u); }
                    } else {
                        const float* pa = aux + (long long)row * g.ldaux + col;
                        if (full) {
                            const f32x4 t0 = *reinterpret_cast<const f32x4*>(pa), t1 = *reinterpret_cast<const f32x4*>(pa + 4);
                            a8[0] = t0.x; a8[1] = t0.y; a8[2] = t0.z; a8[3] = t0.w; a8[4] = t1.x; a8[5] = t1.y; a8[6] = t1.z; a8[7] = t1.w;
                        } else for (int k = 0; k < 8 && col + k < g.N; ++k) a8[k] = pa[k];
                    }
                    if (g.epi == 1) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) o[k] = a8[k] > 0.f ? o[k] : 0.f;
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; ++k) o[k] *= silu_deriv(a8[k]);
                    }
                }
                if (g.colsum) {
                    // the sums of the output AS STORED: a single-plane Cp holds the bf16 rounding of o (a no-op for the rounded product itself and
                    // its ReLU / mask forms; the SiLU-derivative epilogue's products are not bf16 values -- they were summed unrounded before)
#pragma unroll
                    for (int k = 0; k < 8; ++k) cs[k] += (NPL == 1 && Cp) ? rbf(o[k]) : o[k];
                }
                if (C) {
                    float* pc = C + (long long)row * g.ldc + col;
                    if (full) {
                        *reinterpret_cast<f32x4*>(pc) = (f32x4){o[0], o[1], o[2], o[3]};
                        *reinterpret_cast<f32x4*>(pc + 4) = (f32x4){o[4], o[5], o[6], o[7]};
                    } else for (int k = 0; k < 8 && col + k < g.N; ++k) pc[k] = o[k];
                }
                if (Cp) {
                    // the output's own planes: columns past N inside this 8-group are written as zeros (they are k padding of the consumer)
                    u32x4 q0, q1, q2;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float a = col + 2 * k < g.N ? o[2 * k] : 0.f, b = col + 2 * k + 1 < g.N ? o[2 * k + 1] : 0.f;
                        unsigned x0, x1 = 0u, x2 = 0u;
                        if constexpr (NPL == 3) split_pair3(a, b, x0, x1, x2);
                        else x0 = split_pack_rn(a, b);
                        q0[k] = x0; q1[k] = x1; q2[k] = x2;
                    }
                    unsigned short* pp = Cp + (long long)row * g.ldcp + col;
                    *reinterpret_cast<u32x4*>(pp) = q0;
                    if constexpr (NPL == 3) {
                        *reinterpret_cast<u32x4*>(pp + g.pc) = q1;
                        *reinterpret_cast<u32x4*>(pp + 2 * g.pc) = q2;
                    }
                }
            };
            // [r6] The two hot epilogues of the bf16-storage path -- ReLU forward (sign byte + bf16 row) and ReLU gradient from the sign byte -- on
            // whole 8-column groups with the bf16 matrix as the only output.  ReLU and the mask select either keep a value or replace it by +0, so they
            // commute with the rounding: the row is rounded ONCE, by the pack that stores it, and the sign byte / the column sums are read off the
            // packed words.  (The general row rounds, converts back, acts, tests eight column bounds and packs again: ~95 VALU per row -- at 16 rows per
            // thread and two waves per SIMD that is the 8 us the phases tool shows for a 256 x 256 tile: the epilogue was VALU-bound, not store-bound.)
            // Same bits as the general row: tests/test_bf16_gpu.py::test_b16_fast_epilogue_rows_equal_the_general_row.
            const bool fast = NPL == 1 && g.splitk == 1 && Cp != nullptr && C == nullptr && C2 == nullptr && full && g.general_rows == 0 &&
                              ((g.epi == 0 && g.act <= 1) || use_mask);
            auto fast_row = [&](int rl, const f32x4 v0, const f32x4 v1) {
                const int row = m0 + rl;
                float o[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                if (g.epi == 0) {
                    if (g.act == 1) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) o[k] = fmaxf(o[k], 0.f);
                    }
                } else {
                    const unsigned bits = mask8[(long long)row * g.ldm8 + (col >> 3)];
#pragma unroll
                    for (int k = 0; k < 8; ++k) o[k] = ((bits >> k) & 1u) ? o[k] : 0.f;
                }
                u32x4 q;
#pragma unroll
                for (int k = 0; k < 4; ++k) q[k] = split_pack_rn(o[2 * k], o[2 * k + 1]);
                if (g.epi == 0 && g.act == 1 && mask8) {                 // rounded value > 0  <=>  its bf16 magnitude bits are not all zero (after ReLU nothing is negative)
                    unsigned bits = 0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) bits |= ((q[k] & 0x7fffu) ? 1u : 0u) << (2 * k) | ((q[k] & 0x7fff0000u) ? 1u : 0u) << (2 * k + 1);
                    mask8[(long long)row * g.ldm8 + (col >> 3)] = (unsigned char)bits;
                }
                if (g.colsum) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) { cs[2 * k] += split_bitsf(q[k] << 16); cs[2 * k + 1] += split_bitsf(q[k] & 0xffff0000u); }
                }
                *reinterpret_cast<u32x4*>(Cp + (long long)row * g.ldcp + col) = q;
            };
            constexpr int ITER = BM / RPI;
            if (m0 + BM <= g.M) {
                // full tile in M: every image read of the thread's ITER rows is issued before the first row is processed (a rolled loop was one
                // LDS round trip + one store issue per row, end to end: 4.2 us per 256 x 128 half, profiles/r04_gemm_b16_phases.txt)
                f32x4 va[ITER], vb[ITER];
#pragma unroll
                for (int it = 0; it < ITER; ++it) {
                    const int rl = (tid >> 4) + it * RPI;
                    va[it] = *reinterpret_cast<const f32x4*>(sC + rl * XP_CPF + c8);
                    vb[it] = *reinterpret_cast<const f32x4*>(sC + rl * XP_CPF + c8 + 4);
                }
                if (fast) {
#pragma unroll
                    for (int it = 0; it < ITER; ++it) fast_row((tid >> 4) + it * RPI, va[it], vb[it]);
                } else {
#pragma unroll
                    for (int it = 0; it < ITER; ++it) do_row((tid >> 4) + it * RPI, va[it], vb[it]);
                }
            } else {
#pragma unroll 2
                for (int rl = tid >> 4; rl < BM; rl += RPI) {
                    if (m0 + rl >= g.M) break;
                    const f32x4 v0 = *reinterpret_cast<const f32x4*>(sC + rl * XP_CPF + c8), v1 = *reinterpret_cast<const f32x4*>(sC + rl * XP_CPF + c8 + 4);
                    if (fast) fast_row(rl, v0, v1);
                    else do_row(rl, v0, v1);
                }
            }
        }
        if (g.dbg && tid == 0) g.dbg[8 * (blockIdx.y * gridDim.x + blockIdx.x) + 7] = wall_clock64();     // (diagnostics: this thread's stores issued)
        if (g.colsum) {
            // Column sums of the tile as stored (rounded, masked): what pulse_colsum_partial_b16 would compute from the written matrix, taken
            // here while the values are in registers -- the bias gradient of the layer whose dZ this launch produces costs no pass over dZ.
            // The RPI thread rows of a column group are added in row order (fixed tree: deterministic).
            __syncthreads();                                        // every read of the transpose image is done
            float* red = sC;                                        // [RPI][128]
#pragma unroll
            for (int k = 0; k < 8; ++k) red[(tid >> 4) * PBN + c8 + k] = cs[k];
            __syncthreads();
            if (tid < PBN && n0 + tid < g.N) {
                float t = 0.f;
#pragma unroll 8
                for (int r = 0; r < RPI; ++r) t += red[r * PBN + tid];
                g.colsum[bz * g.sColsum + (long long)tm * g.ldcs + n0 + tid] = t;
            }
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------------------
// f(std::bool_constant<AKC>, std::bool_constant<BKC>) for the three supported layout combinations (pulse_gemm_x3p has refused <false, true>)
template <typename F>
auto xp_by_layout(bool akc, bool bkc, F&& f) {
    using T = std::true_type; using N = std::false_type;
    return akc && bkc ? f(T{}, T{}) : akc ? f(T{}, N{}) : f(N{}, N{});
}

// The launchers: ``g`` arrives complete (tiles_m / tiles_n set for the tiling that is launched); all return a PULSE_* code.
// gemm_x3p.hip: gemm_x3p_kernel, 256-row (``big``, three planes only) or 128-row tiles
int launch_gemm_x3p(const XpArgs& g, bool akc, bool bkc, int npl, bool big, hipStream_t stream);
// gemm_b16.hip: single plane, 256-row tiles: the three-stage ring (256 x 128) and the 256 x 256 kernel
int launch_gemm_b16r(const XpArgs& g, bool akc, bool bkc, hipStream_t stream);
int launch_gemm_b16w(const XpArgs& g, bool akc, bool bkc, hipStream_t stream);
inline dim3 xp_grid(const XpArgs& g) { return dim3((unsigned)(g.tiles_m * g.tiles_n), (unsigned)(g.batch * g.splitk)); }

}  // namespace pulse
