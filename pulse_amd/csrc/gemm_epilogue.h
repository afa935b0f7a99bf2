// The epilogue of the fp32-storage GEMM kernels (gemm_f32.hip, gemm_x3.hip, gemm_x3w.hip): everything between "the accumulators are in the LDS
// image" and "the tile is in global memory".  The element math, the general path (ragged tiles, SiLU forms, unaligned pitches) and the ReLU bit-mask
// word handling exist HERE ONLY; the kernels keep what differs between them on purpose: where the fast path's aux loads are placed and the form of
// its bit-mask reader.
//
// The image: the tile's accumulators as fp32 rows of PITCH floats at the start of the dynamic LDS (the staging buffers are free after the main loop),
// 128 columns wide, 8 SWEEPS rows high, image column c holding tile column tile_col(c).  Every global access of the vector paths is then a 16-byte
// access covering 512 contiguous bytes of one row per half-wave, thread = (row slot tid >> 5 of a sweep of 8 rows, image columns 4 (tid & 31) ..).
// Callers pass their thread coordinates: tid, wave (wm, wn) of the 2 x 2 wave grid, half = lane >> 5, l31 = lane & 31.
#pragma once
#include "gemm_shared.h"

namespace pulse {

// ---- element math (silu, silu_deriv, rbf: gemm_shared.h) -----------------------------------------------------------------------------------------
// N elements through EPI 0's activation ``act`` (GemmArgs): o = the accumulators in, C's values out; c2 = what C2 receives from the SiLU forms
// (act 2: the pre-activation, kept for the backward pass if C2 is given; act 3: d silu / d z, which the backward pass multiplies by: EPI 3)
template <int N>
__device__ __forceinline__ void epi_act(int act, float (&o)[N], float (&c2)[N]) {
    if (act == 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) o[k] = fmaxf(o[k], 0.f);
    } else if (act == 2) {
#pragma unroll
        for (int k = 0; k < N; ++k) { c2[k] = o[k]; o[k] = silu(o[k]); }
    } else if (act == 3) {
#pragma unroll
        for (int k = 0; k < N; ++k) { c2[k] = silu_deriv(o[k]); o[k] = silu(o[k]); }
    }
}
// ... and through a gradient epilogue ``epi`` (1 .. 3), a = aux's values
template <int N>
__device__ __forceinline__ void epi_grad(int epi, float (&o)[N], const float (&a)[N]) {
    if (epi == 1) {                                                   // relu-grad: aux = the forward's activations
#pragma unroll
        for (int k = 0; k < N; ++k) o[k] = a[k] > 0.f ? o[k] : 0.f;
    } else if (epi == 3) {                                            // aux = the producer's stored activation derivative
#pragma unroll
        for (int k = 0; k < N; ++k) o[k] *= a[k];
    } else {                                                          // silu-grad: aux = the pre-activation
#pragma unroll
        for (int k = 0; k < N; ++k) o[k] *= silu_deriv(a[k]);
    }
}

// ---- this workgroup's outputs ---------------------------------------------------------------------------------------------------------------------
struct EpiOut {
    float* C; float* C2; const float* aux;
    unsigned* mask;                        // ReLU bit mask: written by the relu forward, read by relu-grad when aux is null (``use_mask``)
    bool use_mask;
};
__device__ __forceinline__ EpiOut epi_out(const GemmArgs& g, int bz, int sp) {
    EpiOut e;
    e.C = g.C + bz * g.sC + sp * g.sSplit;
    e.C2 = g.C2 ? g.C2 + bz * g.sC2 : nullptr;
    e.aux = g.aux ? g.aux + bz * g.sAux : nullptr;
    e.mask = g.mask ? g.mask + bz * g.sMask : nullptr;
    e.use_mask = g.epi == 1 && e.aux == nullptr;
    return e;
}
// full tiles of the epilogues that need no transcendental take a kernel's fast path
__device__ __forceinline__ bool epi_fast_form(const GemmArgs& g) { return g.epi == 1 || g.epi == 3 || (g.epi == 0 && g.act < 2); }

// ---- fast path (full tile): per 16-byte store one ds_read_b128, the activation, one buffer store whose row advance is a scalar offset -- no
// per-access address arithmetic on the VALU.  rsC = the tile's origin in C, voC / ldsC = this thread's byte offsets in C / the image at sweep 0.
// EPI 0 (plain / ReLU / ReLU + mask write): mrow = m0 + (tid >> 5), cg = the thread's column group (mask_word)
template <int PITCH, int SWEEPS, int UNROLL>
__device__ __forceinline__ void epi_fast_act(const GemmArgs& g, unsigned* mask, __amdgpu_buffer_rsrc_t rsC, int voC, int ldsC, int mrow, int cg) {
    const bool relu = g.act == 1;
    const bool wmask = relu && mask != nullptr;
    unsigned w = 0;
#pragma unroll UNROLL
    for (int q = 0; q < SWEEPS; ++q) {
        f32x4 v = lds_read(ldsC + q * 8 * PITCH * 4);
        if (wmask) {
            w |= ((v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u) | (v.z > 0.f ? 4u : 0u) | (v.w > 0.f ? 8u : 0u)) << (4 * (q & 7));
            if ((q & 7) == 7) { mask[mask_word(mrow + 64 * (q >> 3), cg, g.ldmask)] = w; w = 0; }
        }
        if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        buf_store(v, rsC, voC, q * 8 * g.ldc * 4);
    }
}
// one sweep of relu-grad (a = aux's four values, or the +-1 expansion of four mask bits) or multiply-by-aux (``mul``)
__device__ __forceinline__ void epi_fast_grad(bool mul, f32x4 a, int lds_addr, __amdgpu_buffer_rsrc_t rsC, int voC, int soff) {
    f32x4 v = lds_read(lds_addr);
    if (mul) { v.x *= a.x; v.y *= a.y; v.z *= a.z; v.w *= a.w; }
    else { v.x = a.x > 0.f ? v.x : 0.f; v.y = a.y > 0.f ? v.y : 0.f; v.z = a.z > 0.f ? v.z : 0.f; v.w = a.w > 0.f ? v.w : 0.f; }
    buf_store(v, rsC, voC, soff);
}

// ---- general path ---------------------------------------------------------------------------------------------------------------------------------
template <int PITCH, int SWEEPS, typename ColMap>
__device__ __forceinline__ void epi_general(const GemmArgs& g, const EpiOut& e, int tid, int wm, int wn, int half, int l31, int m0, int n0,
                                            ColMap tile_col) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (g.vec_epi) {
        // 16-byte path.  The mask word of a 64-row block is read once at the block's first row slot and stored after its last (rows past M and columns
        // past N contribute zero bits; the buffer covers roundup64(M) rows).
        const int c4 = (tid & 31) * 4, rl0 = tid >> 5;
        const int col = n0 + tile_col(c4);
        if (col >= g.N) return;
        const bool full = col + 3 < g.N;
        const bool wmask = g.epi == 0 && g.act == 1 && e.mask != nullptr;
        unsigned w = 0;
        auto store4 = [&](float* p, const float (&x)[4]) {                 // four values to columns col .. col + 3 of a row (p: column col of it)
            if (full) *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
            else for (int k = 0; k < 4 && col + k < g.N; ++k) p[k] = x[k];
        };
        auto word = [&](int q) { return mask_word(m0 + 64 * (q >> 3) + rl0, col >> 2, g.ldmask); };     // of sweep q's 64-row block
#pragma unroll 4
        for (int q = 0; q < SWEEPS; ++q) {
            const int rl = rl0 + 8 * q;
            const int row = m0 + rl;
            if (e.use_mask && (q & 7) == 0 && m0 + 64 * (q >> 3) < g.M) w = e.mask[word(q)];
            if (row >= g.M) {
                if (wmask && (q & 7) == 7 && m0 + 64 * (q >> 3) < g.M) { e.mask[word(q)] = w; w = 0; }
                continue;
            }
            const float4 v = *reinterpret_cast<const float4*>(smem + rl * PITCH + c4);
            float o[4] = {v.x, v.y, v.z, v.w};
            if (wmask) {
#pragma unroll
                for (int k = 0; k < 4; ++k) w |= (col + k < g.N && o[k] > 0.f ? 1u : 0u) << (4 * (q & 7) + k);
                if ((q & 7) == 7) { e.mask[word(q)] = w; w = 0; }
            }
            if (e.use_mask) {
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = ((w >> (4 * (q & 7) + k)) & 1u) ? o[k] : 0.f;
                store4(e.C + (long long)row * g.ldc + col, o);
                continue;
            }
            if (g.epi == 0) {
                float d[4];
                epi_act(g.act, o, d);
                if (g.act >= 2 && e.C2) store4(e.C2 + (long long)row * g.ldc2 + col, d);
            } else {
                const float* pa = e.aux + (long long)row * g.ldaux + col;
                float a4[4] = {0.f, 0.f, 0.f, 0.f};
                if (full) { const float4 t = *reinterpret_cast<const float4*>(pa); a4[0] = t.x; a4[1] = t.y; a4[2] = t.z; a4[3] = t.w; }
                else for (int k = 0; k < 4 && col + k < g.N; ++k) a4[k] = pa[k];
                epi_grad(g.epi, o, a4);
            }
            store4(e.C + (long long)row * g.ldc + col, o);
        }
        return;
    }
    // Scalar path (unaligned C / aux pitches: odd test shapes, not the training shapes): one dword per lane, read back from the same image -- the
    // accumulator registers are dead in EVERY path (live across this path's per-element address arithmetic, the weight-gradient instantiation of
    // the fp32 MFMA kernel once spilled 351 VGPRs).  Which thread stores an element is invisible in the result; the map is written in the wave / lane
    // coordinates the kernels hold anyway (2 x 2 waves, wave (wm, wn): the image's row half wm, columns wn 64 + {0, 32} + l31; in the 128-row kernels
    // that is the lane's own accumulator elements), so the path adds no per-thread value for the register allocator to carry.
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {
        const int c = wn * 64 + j * 32 + l31;
        const int col = n0 + tile_col(c);
        if (col >= g.N) continue;
        for (int i = 0; i < SWEEPS / 8; ++i) {
#pragma unroll 1
            for (int r = 0; r < 16; ++r) {
                const int rl = wm * 4 * SWEEPS + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const int row = m0 + rl;
                if (row >= g.M) continue;
                float v[1] = {smem[rl * PITCH + c]};
                if (g.epi == 0) {
                    float d[1];
                    epi_act(g.act, v, d);
                    if (g.act >= 2 && e.C2) e.C2[(long long)row * g.ldc2 + col] = d[0];
                } else {
                    const float a[1] = {e.aux[(long long)row * g.ldaux + col]};
                    epi_grad(g.epi, v, a);
                }
                e.C[(long long)row * g.ldc + col] = v[0];
            }
        }
    }
}

// ---- the 128-row kernels' epilogue (WM = 32-row MFMA tiles per wave: tile height 64 WM; 4 waves as 2 x 2, each WM x 2 MFMA tiles) --------------------
// C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
template <int WM>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& g, f32x16 (&acc)[WM][2], int tid, int m0, int n0, int bz, int sp, int wm, int wn,
                                              int half, int l31) {
    if (g.round_bf16) {
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = rbf(acc[i][j][r]);
    }
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // The tile origin and the batch / split indices are made opaque here, so that none of the epilogue's address arithmetic is merged with the
    // prologue's uses of them and carried in SGPRs across the main loop (these kernels run at the SGPR limit: the bf16 dX form spills 19 with this
    // line, 26 without; no instruction is emitted).
    asm volatile("" : "+s"(m0), "+s"(n0), "+s"(bz), "+s"(sp));
    const EpiOut e = epi_out(g, bz, sp);
    const bool fast = g.vec_epi && m0 + 64 * WM <= g.M && n0 + BN <= g.N && epi_fast_form(g);
    const int c4 = (tid & 31) * 4;
    const int rl0 = tid >> 5;
    f32x4 ax[8 * WM];
    unsigned mw[WM];                           // this thread's mask words: rows rl0 + 8 q of 64-row block b = q / 8, columns c4 .. c4 + 3
    if (fast && e.use_mask) {
#pragma unroll
        for (int b = 0; b < WM; ++b) mw[b] = e.mask[mask_word(m0 + 64 * b + rl0, (n0 + c4) >> 2, g.ldmask)];
        // [r6, last hours] The bits are expanded HERE into the registers the aux path would have loaded (+1 / -1 per element) and the store loop
        // below is the aux path's.  The loop this replaces -- ``nb = mw >> 4 q; v.x = (nb & 1) ? v.x : 0`` after the barrier -- was bit-identical in
        // every test and returned garbage in 12 - 48 elements of a row now and then as soon as another stream's or process's GEMMs ran beside the
        // launch (tools/gemm_contend_probe.py: 5 412 wrong elements in 4 000 launches, 0 alone, 0 for the aux path); this form:
        // 0 in 3 000, and the agent-level tests pass 10 / 10 beside a GEMM-hammering process with the masks forced on.
#pragma unroll
        for (int q = 0; q < 8 * WM; ++q) {
            const unsigned nb = mw[q >> 3] >> (4 * (q & 7));
            ax[q] = (f32x4){(nb & 1u) ? 1.f : -1.f, (nb & 2u) ? 1.f : -1.f, (nb & 4u) ? 1.f : -1.f, (nb & 8u) ? 1.f : -1.f};
        }
    } else if (fast && g.epi != 0) {           // relu-grad / multiply-by-aux: the 16 aux loads fly while the accumulators go through LDS
        const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(e.aux) + (long long)m0 * g.ldaux + n0, 0,
                                                                            0xffffffffu, RSRC_FLAGS);
        const int voX = (rl0 * g.ldaux + c4) * 4;
#pragma unroll
        for (int q = 0; q < 8 * WM; ++q) ax[q] = buf_load(rsX, voX, q * 8 * g.ldaux * 4);
    }
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                smem[(wm * 32 * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * CP + wn * 64 + j * 32 + l31] = acc[i][j][r];
    __syncthreads();
    if (g.dbg && tid == 0) g.dbg[8 * (blockIdx.y * gridDim.x + blockIdx.x) + 6] = clock64();
    if (!fast) return epi_general<CP, 8 * WM>(g, e, tid, wm, wn, half, l31, m0, n0, [](int c) { return c; });
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc(e.C + (long long)m0 * g.ldc + n0, 0, 0xffffffffu, RSRC_FLAGS);
    const int voC = (rl0 * g.ldc + c4) * 4;
    const int ldsC = (rl0 * CP + c4) * 4;
    if (g.epi == 0) {
        epi_fast_act<CP, 8 * WM, 8 * WM>(g, e.mask, rsC, voC, ldsC, m0 + rl0, (n0 + c4) >> 2);
    } else if (g.epi == 1) {                   // relu-grad: aux = the activations, or the +-1 expansion of the forward's bit mask (above)
#pragma unroll
        for (int q = 0; q < 8 * WM; ++q) epi_fast_grad(false, ax[q], ldsC + q * 8 * CP * 4, rsC, voC, q * 8 * g.ldc * 4);
    } else {                                   // EPI_MUL_AUX
#pragma unroll
        for (int q = 0; q < 8 * WM; ++q) epi_fast_grad(true, ax[q], ldsC + q * 8 * CP * 4, rsC, voC, q * 8 * g.ldc * 4);
    }
}

}  // namespace pulse
