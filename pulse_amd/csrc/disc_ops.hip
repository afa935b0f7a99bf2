// The AMP discriminator's head kernels on gfx950 (HBM- or latency-bound glue around its GEMMs).  Compiled with -ffp-contract=off.
// disc_head, disc_penalty, disc_reg (AMPAgent._disc_loss) and disc_reward (AMPAgent._calc_disc_rewards).
#include "common.h"

namespace pulse {

// AMPAgent._disc_loss head (phc/learning/amp_agent.py:895-952) on the logits of the 3b stacked rows [agent | replay | demo]:
// prediction loss 0.5 (BCEWithLogits(agent U replay, 0) + BCEWithLogits(demo, 1)), its gradient w.r.t. every logit (times
// ``scale`` = disc_coef / world_size), the two accuracies and the two logit means -- one launch instead of ~45 tiny tensor ops and an
// autograd pass per minibatch.  One workgroup: 3b logits are a few hundred KB; reductions in double, fixed order.
__global__ void __launch_bounds__(1024) disc_head_kernel(const float* __restrict__ logits, long long ls, int b, float scale, float* __restrict__ dlogits, long long ds,
                                                         float* __restrict__ stats, unsigned short* __restrict__ dl16, long long ds16, float* __restrict__ bias_grad) {
    __shared__ double red[16][7];
    const int n = 3 * b, na = 2 * b;
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; // BCE agent, BCE demo, #agent < 0, #demo > 0, sum agent logit, sum demo logit, sum of d loss / d logit
    const float ga = scale * 0.5f / (float)na, gd = scale * 0.5f / (float)b;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const float x = logits[(long long)i * ls];
        const float sp = fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));        // softplus(x) = BCEWithLogits(x, 0); BCE(x, 1) = softplus(x) - x
        const float sg = 1.f / (1.f + expf(-x));
        if (i < na) {
            acc[0] += (double)sp; acc[2] += x < 0.f ? 1.0 : 0.0; acc[4] += (double)x;
            const float gl = ga * sg;
            if (dlogits) dlogits[(long long)i * ds] = gl;
            const unsigned q = split_pack_rn(gl, 0.f) & 0xffffu;
            if (dl16) dl16[(long long)i * ds16] = (unsigned short)q;
            acc[6] += dl16 ? (double)split_bitsf(q << 16) : (double)gl;      // the logit bias' gradient sums what the backward pass reads
        } else {
            acc[1] += (double)(sp - x); acc[3] += x > 0.f ? 1.0 : 0.0; acc[5] += (double)x;
            const float gl = gd * (sg - 1.f);
            if (dlogits) dlogits[(long long)i * ds] = gl;
            const unsigned q = split_pack_rn(gl, 0.f) & 0xffffu;
            if (dl16) dl16[(long long)i * ds16] = (unsigned short)q;
            acc[6] += dl16 ? (double)split_bitsf(q << 16) : (double)gl;
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) acc[k] = lane_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) red[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[7];
        for (int k = 0; k < 7; ++k) { t[k] = 0.0; for (int w = 0; w < 16; ++w) t[k] += red[w][k]; }
        if (bias_grad) *bias_grad = (float)t[6];
        const double la = t[0] / na, ld = t[1] / b;
        stats[0] = (float)(0.5 * (la + ld)); stats[1] = (float)la; stats[2] = (float)ld;
        stats[3] = (float)(t[2] / na); stats[4] = (float)(t[3] / b); stats[5] = (float)(t[4] / na); stats[6] = (float)(t[5] / b); stats[7] = 0.f;
    }
}

// AMPAgent._disc_loss gradient penalty (amp_agent.py:925-934): dg = scale * G (fp32 and / or bf16) starts the penalty's backward pass, partials[block] = sum of G^2 over the block's elements.  G is (rows, ld) with its pad columns zero.
__global__ void __launch_bounds__(256) disc_penalty_kernel(const float* __restrict__ G, long long ldg, int rows, int cols4, float scale, float* __restrict__ out32,
                                                          long long ld32, unsigned short* __restrict__ out16, long long ld16, float* __restrict__ partials) {
    __shared__ float red[4];
    float acc = 0.f;
    const long long total = (long long)rows * cols4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / cols4), c = (int)(i - (long long)r * cols4) * 4;
        const float4 v = *reinterpret_cast<const float4*>(G + (long long)r * ldg + c);
        acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        const float a = v.x * scale, b = v.y * scale, cc = v.z * scale, d = v.w * scale;
        if (out32) *reinterpret_cast<float4*>(out32 + (long long)r * ld32 + c) = make_float4(a, b, cc, d);
        if (out16) *reinterpret_cast<uint2*>(out16 + (long long)r * ld16 + c) = make_uint2(split_pack_rn(a, b), split_pack_rn(cc, d));
    }
    acc = lane_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

struct DiscRegArgs { long long off[4]; long long len[4]; float alpha[4]; int n; };

// disc_logit_reg / disc_weight_decay gradient terms (amp_agent.py:919-923, 936-940) over up to four parameter ranges:
// grad[off_r + i] += alpha_r * flat[off_r + i];  partials[block * 4 + r] = sum over the block's share of flat[range r]^2
__global__ void __launch_bounds__(256) disc_reg_kernel(const float* __restrict__ flat, float* __restrict__ grad, const DiscRegArgs a, float* __restrict__ partials) {
    __shared__ float red[4][4];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r >= a.n) break;
        const float* w = flat + a.off[r];
        float* g = grad ? grad + a.off[r] : nullptr;
        const float al = a.alpha[r];
        if (((a.off[r] | a.len[r]) & 3) == 0) {                          // 16-byte path (every weight matrix of a ParamBook)
            const long long n4 = a.len[r] >> 2;
            const bool upd = g && al != 0.f;
            for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
                const float4 v = reinterpret_cast<const float4*>(w)[i];
                acc[r] += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
                if (upd) {
                    float4 t = reinterpret_cast<float4*>(g)[i];
                    t.x += al * v.x; t.y += al * v.y; t.z += al * v.z; t.w += al * v.w;
                    reinterpret_cast<float4*>(g)[i] = t;
                }
            }
            continue;
        }
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.len[r]; i += (long long)gridDim.x * 256) {
            const float v = w[i];
            acc[r] += v * v;
            if (g && al != 0.f) g[i] += al * v;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        acc[r] = lane_sum(acc[r]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][r] = acc[r];
    }
    __syncthreads();
    if (threadIdx.x < 4) partials[blockIdx.x * 4 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// AMPAgent._calc_disc_rewards (amp_agent.py:1027-1041): -log(max(1 - sigmoid(logit), 1e-4)) * scale
__global__ void __launch_bounds__(256) disc_reward_kernel(const float* __restrict__ logits, long long ls, long long n, float scale, float* __restrict__ out, long long os) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = logits[i * ls];
    const float prob = 1.f / (1.f + expf(-x));                          // the reference's op sequence, op for op (amp_agent.py:1033-1038)
    out[i * os] = -logf(fmaxf(1.f - prob, 0.0001f)) * scale;
}

}  // namespace pulse

using namespace pulse;

extern "C" {

int pulse_disc_head(const float* logits, int64_t logit_stride, int32_t b, float scale, float* dlogits, int64_t dlogit_stride, float* stats, pulse_stream_t s) {
    PULSE_REQUIRE(b >= 1 && logit_stride >= 1 && dlogit_stride >= 1, "pulse_disc_head: bad sizes");
    PULSE_REQUIRE(logits && dlogits && stats, "pulse_disc_head: null pointer");
    hipLaunchKernelGGL(disc_head_kernel, dim3(1), dim3(1024), 0, as_stream(s), logits, (long long)logit_stride, b, scale, dlogits, (long long)dlogit_stride, stats,
                       (unsigned short*)nullptr, 0LL, (float*)nullptr);
    return check_launch("pulse_disc_head");
}

int pulse_disc_head_b16(const float* logits, int64_t logit_stride, int32_t b, float scale, float* dlogits, int64_t dlogit_stride, void* dlogits16,
                        int64_t dlogit16_stride, float* stats, float* bias_grad, pulse_stream_t s) {
    PULSE_REQUIRE(b >= 1 && logit_stride >= 1, "pulse_disc_head_b16: bad sizes");
    PULSE_REQUIRE(logits && stats && (dlogits || dlogits16), "pulse_disc_head_b16: null pointer");
    PULSE_REQUIRE((!dlogits || dlogit_stride >= 1) && (!dlogits16 || dlogit16_stride >= 1), "pulse_disc_head_b16: bad strides");
    hipLaunchKernelGGL(disc_head_kernel, dim3(1), dim3(1024), 0, as_stream(s), logits, (long long)logit_stride, b, scale, dlogits, (long long)dlogit_stride, stats,
                       reinterpret_cast<unsigned short*>(dlogits16), (long long)dlogit16_stride, bias_grad);
    return check_launch("pulse_disc_head_b16");
}

int pulse_disc_penalty(const float* g, int64_t ldg, int32_t rows, int32_t cols, float scale, float* out32, int64_t ld32, void* out16, int64_t ld16, float* partials,
                       int32_t num_blocks, pulse_stream_t s) {
    PULSE_REQUIRE(rows >= 1 && cols >= 1 && num_blocks >= 1, "pulse_disc_penalty: bad sizes");
    PULSE_REQUIRE(g && partials, "pulse_disc_penalty: null pointer");
    PULSE_REQUIRE((cols % 4) == 0 && (ldg % 4) == 0 && ldg >= cols && (reinterpret_cast<uintptr_t>(g) & 15) == 0,
                  "pulse_disc_penalty: cols / pitch must be multiples of 4 floats (the pad columns of G are zero and are processed with it)");
    PULSE_REQUIRE(!out32 || ((ld32 % 4) == 0 && ld32 >= cols && (reinterpret_cast<uintptr_t>(out32) & 15) == 0), "pulse_disc_penalty: fp32 output rows must be 16-byte aligned");
    PULSE_REQUIRE(!out16 || ((ld16 % 4) == 0 && ld16 >= cols && (reinterpret_cast<uintptr_t>(out16) & 7) == 0), "pulse_disc_penalty: bf16 output rows must be 8-byte aligned");
    hipLaunchKernelGGL(disc_penalty_kernel, dim3((unsigned)num_blocks), dim3(256), 0, as_stream(s), g, (long long)ldg, rows, cols / 4, scale, out32, (long long)ld32,
                       reinterpret_cast<unsigned short*>(out16), (long long)ld16, partials);
    return check_launch("pulse_disc_penalty");
}

int pulse_disc_reg(const float* flat, float* grad, int32_t num_ranges, const int64_t* offsets, const int64_t* lengths, const float* alphas, float* partials,
                   int32_t num_blocks, pulse_stream_t s) {
    PULSE_REQUIRE(num_ranges >= 1 && num_ranges <= 4 && num_blocks >= 1, "pulse_disc_reg: 1..4 ranges");
    PULSE_REQUIRE(flat && offsets && lengths && alphas && partials, "pulse_disc_reg: null pointer");
    PULSE_REQUIRE((reinterpret_cast<uintptr_t>(flat) & 15) == 0 && (!grad || (reinterpret_cast<uintptr_t>(grad) & 15) == 0), "pulse_disc_reg: flat / grad must be 16-byte aligned");
    DiscRegArgs a;
    a.n = num_ranges;
    for (int r = 0; r < 4; ++r) {
        a.off[r] = r < num_ranges ? offsets[r] : 0; a.len[r] = r < num_ranges ? lengths[r] : 0; a.alpha[r] = r < num_ranges ? alphas[r] : 0.f;
        PULSE_REQUIRE(a.off[r] >= 0 && a.len[r] >= 0, "pulse_disc_reg: negative range");
    }
    hipLaunchKernelGGL(disc_reg_kernel, dim3((unsigned)num_blocks), dim3(256), 0, as_stream(s), flat, grad, a, partials);
    return check_launch("pulse_disc_reg");
}

int pulse_disc_reward(const float* logits, int64_t logit_stride, int64_t n, float scale, float* out, int64_t out_stride, pulse_stream_t s) {
    PULSE_REQUIRE(n >= 0, "pulse_disc_reward: negative size");
    if (n == 0) return PULSE_OK;
    PULSE_REQUIRE(logits && out && logit_stride >= 1 && out_stride >= 1, "pulse_disc_reward: bad arguments");
    hipLaunchKernelGGL(disc_reward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(s), logits, (long long)logit_stride, (long long)n, scale, out,
                       (long long)out_stride);
    return check_launch("pulse_disc_reward");
}
}
