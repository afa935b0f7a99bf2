// What the learner-side translation units (rms_normalize, policy_ops, optim_ops, disc_ops) share: the formulas of the PPO update as device
// functions, one spelling each, and the serial block sum.  Every caller is compiled with -ffp-contract=off; the expressions and their order
// are what the bit-exact tests pin.
#pragma once
#include "common.h"

namespace pulse {

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// ---- RunningMeanStd.forward on one element (phc/utils/running_mean_std.py:96-109): mode 0 normalises, mode 1 un-normalises ----------------------
__device__ __forceinline__ float rms_den(double var, float eps) { return sqrtf((float)var + eps); }
__device__ __forceinline__ float rms_apply(float v, float mu, float den, float clip, int mode) {
    return mode == 0 ? clampf((v - mu) / den, -clip, clip) : den * clampf(v, -clip, clip) + mu;
}

// ---- the Gaussian head: 16 lanes per sample, each lane walks columns l, l + 16, ... ------------------------------------------------------------
constexpr int kLanesPerSample = 16;
constexpr float kHalfLog2Pi = 0.91893853320467274178f;  // 0.5 * ln(2 pi)

// Normal(mu, exp(logstd)) neglogp from the row sums of ((a - mu) / sigma)^2 and of logstd
__device__ __forceinline__ float gauss_neglogp(float quad, int A, float lsum) { return 0.5f * quad + kHalfLog2Pi * (float)A + lsum; }

// what the PPO loss needs of an action column: sigma, sigma^2 and the two column terms of rl_games' policy_kl(p0 = new, p1 = old)
struct GaussCol { float sg, sg2, klog, kden; };
__device__ __forceinline__ GaussCol gauss_col(float logstd, float old_logstd) {
    const float sg = expf(logstd), s1 = expf(old_logstd);
    return GaussCol{sg, sg * sg, logf(s1 / sg + 1e-5f), 2.0f * (s1 * s1 + 1e-5f)};
}

// one element's terms of the neglogp quadratic, the bound loss and the KL, added onto the lane's sums; returns action - mu
__device__ __forceinline__ float gauss_loss_terms(const GaussCol& c, float m, float act, float old_m, bool bounds, float& quad, float& bl, float& kl) {
    const float da = act - m;
    const float zz = da / c.sg;
    quad += zz * zz;
    if (bounds) {
        const float hi = fmaxf(m - 1.0f, 0.f), lo = fminf(m + 1.0f, 0.f);
        bl += lo * lo + hi * hi;
    }
    const float dm = old_m - m;
    kl += c.klog + (c.sg2 + dm * dm) / c.kden + (-0.5f);
    return da;
}

// d loss / d mu of one element (before the 1 / batch): the neglogp path and the bound loss
__device__ __forceinline__ float gauss_dmu(float g_nlp, float da, float sg2, float m, bool bounds, float bounds_coef) {
    float gmu = g_nlp * (-da / sg2);
    if (bounds) gmu += bounds_coef * (2.0f * fmaxf(m - 1.0f, 0.f) + 2.0f * fminf(m + 1.0f, 0.f));
    return gmu;
}
// ... stored as fp32 and, where the bf16-storage path asks for it, as bf16
__device__ __forceinline__ void store_f32_b16(float* out32, void* out16, long long at16, float g) {
    *out32 = g;
    if (out16) reinterpret_cast<unsigned short*>(out16)[at16] = (unsigned short)(split_pack_rn(g, 0.f) & 0xffffu);
}

// the per-sample scalar part of _actor_loss / _critic_loss (phc/learning/common_agent.py:564-587) with its gradients: g_nlp = d a_loss / d neglogp,
// g_v = critic_coef * d c_loss / d value (both before the 1 / batch)
struct PpoSample { float a_loss, c_loss, clipped, g_nlp, g_v; };
__device__ __forceinline__ PpoSample ppo_sample_terms(float nlp, float adv, float old_nlp, float v, float old_v, float ret, float e_clip, int clip_value,
                                                      float critic_coef) {
    PpoSample o;
    const float ratio = expf(old_nlp - nlp);
    const float rc = clampf(ratio, 1.0f - e_clip, 1.0f + e_clip);
    const float l1 = -(adv * ratio), l2 = -(adv * rc);
    o.a_loss = fmaxf(l1, l2);
    // d a_loss / d ratio: -adv where the unclipped branch is active (or tied inside the clip range)
    const bool inside = (ratio >= 1.0f - e_clip) && (ratio <= 1.0f + e_clip);
    const float g_ratio = (inside || l1 > l2) ? -adv : 0.f;
    o.g_nlp = g_ratio * (-ratio);                                // d ratio / d nlp = -ratio
    o.clipped = fabsf(ratio - 1.0f) > e_clip ? 1.f : 0.f;
    float g_v;
    if (clip_value) {
        const float dv = v - old_v;
        const float vpc = old_v + clampf(dv, -e_clip, e_clip);
        const float e1 = (v - ret) * (v - ret), e2 = (vpc - ret) * (vpc - ret);
        o.c_loss = fmaxf(e1, e2);
        if (e1 >= e2) g_v = 2.0f * (v - ret);
        else g_v = (fabsf(dv) <= e_clip) ? 2.0f * (vpc - ret) : 0.f;
    } else {
        o.c_loss = (ret - v) * (ret - v);
        g_v = -2.0f * (ret - v);
    }
    o.g_v = critic_coef * g_v;
    return o;
}

// ---- the serial block sum of N values at once: wave butterfly, red[value][wave], one barrier, thread 0 adds in wave order (left to right) ------
// total[] is valid in thread 0 only.  red is of the type the sum is carried in (adam_body sums doubles and adds their float roundings).
// NOT the pairwise (red[0] + red[1]) + (red[2] + red[3]) of disc_penalty / disc_reg / reduce_grads: another association, pinned by its own tests.
template <int N, int WAVES, typename R, typename T>
__device__ __forceinline__ void block_sum(const T (&v)[N], R (&red)[N][WAVES], R (&total)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const T s = lane_sum(v[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = (R)s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        total[k] = threadIdx.x == 0 ? red[k][0] : R(0);
#pragma unroll
        for (int w = 1; w < WAVES; ++w) if (threadIdx.x == 0) total[k] += red[k][w];
    }
}
template <int WAVES, typename R, typename T>
__device__ __forceinline__ R block_sum(T v, R (&red)[1][WAVES]) {                // one value
    const T a[1] = {v};
    R t[1];
    block_sum(a, red, t);
    return t[0];
}

}  // namespace pulse
