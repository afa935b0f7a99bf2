// The Gaussian policy head of the PPO update on gfx950 (latency-bound; formulas in learner_math.h):
//   policy_sample                rl_games ModelA2CContinuousLogStd eval branch + value un-normalise (phc/learning/common_agent.py:262-288)
//   ppo_loss                     _actor_loss/_critic_loss/bound_loss + neglogp + policy_kl and their analytic gradients (:400-491,512-520,564-587)
//   advantage_moments/normalize  _calc_advs (:589-599)
// Compiled with -ffp-contract=off.
#include "learner_math.h"

namespace pulse {

// rollout (eval) branch.  16 lanes per sample.
__global__ void __launch_bounds__(256) policy_sample_kernel(const float* __restrict__ mu, long long mu_stride, const float* __restrict__ logstd,
                                                           const float* __restrict__ noise, long long noise_stride, const float* __restrict__ value_raw,
                                                           long long value_stride, const double* __restrict__ vmean, const double* __restrict__ vvar, int rows, int A,
                                                           float* __restrict__ actions, long long actions_stride, float* __restrict__ sigmas, long long sigmas_stride,
                                                           float* __restrict__ neglogp, long long neglogp_stride, float* __restrict__ values, long long values_stride,
                                                           float* __restrict__ mus_out, long long mus_out_stride) {
    const int g = (blockIdx.x * 256 + threadIdx.x) / kLanesPerSample;
    const int l = threadIdx.x % kLanesPerSample;
    if (g >= rows) return;
    float quad = 0.f, lsum = 0.f;
    for (int j = l; j < A; j += kLanesPerSample) {
        const float ls = logstd[j];
        const float sg = expf(ls);
        const float m = mu[(long long)g * mu_stride + j];
        const float a = m + sg * noise[(long long)g * noise_stride + j];   // Normal(mu, sigma).sample()
        const float zz = (a - m) / sg;
        quad += zz * zz;
        lsum += ls;
        actions[(long long)g * actions_stride + j] = a;
        if (mus_out) mus_out[(long long)g * mus_out_stride + j] = m;
        if (sigmas) sigmas[(long long)g * sigmas_stride + j] = m * 0.0f + sg;   // amp_network_builder.py:142-148
    }
    quad = lane_sum<kLanesPerSample>(quad);
    lsum = lane_sum<kLanesPerSample>(lsum);
    if (l == 0) {
        neglogp[(long long)g * neglogp_stride] = gauss_neglogp(quad, A, lsum);
        if (values) {
            float v = value_raw[(long long)g * value_stride];
            if (vmean) v = rms_apply(v, (float)vmean[0], rms_den(vvar[0], 1e-5f), 5.f, 1);
            values[(long long)g * values_stride] = v;
        }
    }
}

// PPO losses + gradients w.r.t. (mu, value).  16 lanes per sample, 16 samples per 256-thread block.
// HOIST [r6]: what depends on the action column only -- gauss_col: sigma = exp(logstd), sigma^2, the KL's log(s1 / sigma + 1e-5) and 2 (s1^2 + 1e-5) --
// and the row sum of logstd are evaluated once per lane instead of once per sample (three exp, a log and a divide per element were two thirds of the
// kernel's instructions), and a sample's mu / action values stay in registers between the loss pass and the gradient pass.  The plain form, which stays
// for num_actions > 16 * kLossCols, calls the same functions per element: same expressions on the same values in the same order, bit-identical results.
constexpr int kLossCols = 10;          // hoisted columns per lane: num_actions <= 160 (SMPL 69, SMPL-X 153)

template <bool HOIST>
__global__ void __launch_bounds__(256) ppo_loss_kernel(const pulse_ppo_loss_args a) {
    __shared__ float red[5][16];
    const int samples_per_block = 256 / kLanesPerSample;
    const int slot = threadIdx.x / kLanesPerSample;
    const int l = threadIdx.x % kLanesPerSample;
    const int A = a.num_actions;
    const float invB = 1.0f / (float)a.rows;
    float acc_a = 0.f, acc_c = 0.f, acc_b = 0.f, acc_clip = 0.f, acc_kl = 0.f;
    GaussCol col[kLossCols];
    float c_lsum = 0.f;
    if constexpr (HOIST) {
#pragma unroll
        for (int t = 0; t < kLossCols; ++t) {
            const int j = l + kLanesPerSample * t;
            col[t] = GaussCol{1.f, 1.f, 0.f, 1.f};
            if (j < A) {
                const float ls = a.logstd[j];
                col[t] = gauss_col(ls, a.old_logstd[j]);
                c_lsum += ls;
            }
        }
        c_lsum = lane_sum<kLanesPerSample>(c_lsum);
    }
    for (int base = blockIdx.x * samples_per_block; base < a.rows; base += gridDim.x * samples_per_block) {
        const int i = base + slot;
        if (i >= a.rows) continue;
        const long long d = a.idx ? a.idx[i] : (long long)i;
        const float* mu = a.mu + (long long)i * a.mu_stride;
        const float* act = a.actions + d * a.actions_stride;
        const float* omu = a.old_mu + d * a.old_mu_stride;
        float quad = 0.f, lsum = 0.f, bl = 0.f, kl = 0.f;
        float r_m[kLossCols], r_da[kLossCols];                  // HOIST: mu and (action - mu) of this lane's columns
        if constexpr (HOIST) {
            float r_o[kLossCols];
#pragma unroll
            for (int t = 0; t < kLossCols; ++t) {               // all loads of the sample first: one memory round trip, not one per column
                const int j = l + kLanesPerSample * t;
                r_m[t] = 0.f; r_da[t] = 0.f; r_o[t] = 0.f;
                if (j < A) { r_m[t] = mu[j]; r_da[t] = act[j]; r_o[t] = omu[j]; }
            }
#pragma unroll
            for (int t = 0; t < kLossCols; ++t)
                if (l + kLanesPerSample * t < A) r_da[t] = gauss_loss_terms(col[t], r_m[t], r_da[t], r_o[t], a.has_bounds_loss, quad, bl, kl);
            lsum = c_lsum;
        } else {
            for (int j = l; j < A; j += kLanesPerSample) {
                const float ls = a.logstd[j];
                gauss_loss_terms(gauss_col(ls, a.old_logstd[j]), mu[j], act[j], omu[j], a.has_bounds_loss, quad, bl, kl);
                lsum += ls;
            }
            lsum = lane_sum<kLanesPerSample>(lsum);
        }
        quad = lane_sum<kLanesPerSample>(quad); bl = lane_sum<kLanesPerSample>(bl); kl = lane_sum<kLanesPerSample>(kl);
        const PpoSample ps = ppo_sample_terms(gauss_neglogp(quad, A, lsum), a.advantages[d], a.old_neglogp[d], a.value[(long long)i * a.value_stride],
                                              a.clip_value ? a.old_values[d] : 0.f, a.returns[d], a.e_clip, a.clip_value, a.critic_coef);
        // gradients (mean over the batch folded in)
        const auto put_dmu = [&](int j, float da, float sg2, float m) {
            store_f32_b16(a.dmu + (long long)i * a.dmu_stride + j, a.dmu16, (long long)i * a.dmu16_stride + j,
                          gauss_dmu(ps.g_nlp, da, sg2, m, a.has_bounds_loss, a.bounds_loss_coef) * invB);
        };
        if constexpr (HOIST) {
#pragma unroll
            for (int t = 0; t < kLossCols; ++t)
                if (l + kLanesPerSample * t < A) put_dmu(l + kLanesPerSample * t, r_da[t], col[t].sg2, r_m[t]);
        } else {
            for (int j = l; j < A; j += kLanesPerSample) put_dmu(j, act[j] - mu[j], gauss_col(a.logstd[j], a.old_logstd[j]).sg2, mu[j]);
        }
        if (l == 0) {
            store_f32_b16(a.dvalue + (long long)i * a.dvalue_stride, a.dvalue16, (long long)i * a.dvalue16_stride, ps.g_v * invB);
            acc_a += ps.a_loss; acc_c += ps.c_loss; acc_b += bl; acc_clip += ps.clipped; acc_kl += kl;
        }
    }
    if (l == 0) { red[0][slot] = acc_a; red[1][slot] = acc_c; red[2][slot] = acc_b; red[3][slot] = acc_clip; red[4][slot] = acc_kl; }
    __syncthreads();
    if (threadIdx.x < 8) {
        float s = 0.f;
        if (threadIdx.x < 5)
            for (int k = 0; k < 16; ++k) s += red[threadIdx.x][k];
        a.partials[(long long)blockIdx.x * 8 + threadIdx.x] = s;
    }
}

__global__ void __launch_bounds__(256) adv_moments_kernel(const float* __restrict__ ret, const float* __restrict__ val, long long count, float* __restrict__ adv,
                                                         double* __restrict__ partials) {
    __shared__ double red[2][4];
    double s[2] = {0.0, 0.0}, t[2];
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const float a = ret[i] - val[i];
        adv[i] = a;
        s[0] += (double)a; s[1] += (double)a * (double)a;
    }
    block_sum(s, red, t);
    if (threadIdx.x == 0) { partials[2 * blockIdx.x] = t[0]; partials[2 * blockIdx.x + 1] = t[1]; }
}

__global__ void __launch_bounds__(256) adv_normalize_kernel(float* __restrict__ adv, long long count, const double* __restrict__ partials, int nblk) {
    __shared__ float s_mean, s_den;
    if (threadIdx.x == 0) {
        double s1 = 0.0, s2 = 0.0;
        for (int b = 0; b < nblk; ++b) { s1 += partials[2 * b]; s2 += partials[2 * b + 1]; }
        const double n = (double)count;
        const double m = s1 / n;
        double var = (s2 - n * m * m) / (n - 1.0);
        if (var < 0.0) var = 0.0;
        s_mean = (float)m;
        s_den = (float)sqrt(var) + 1e-8f;
    }
    __syncthreads();
    const float m = s_mean, den = s_den;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) adv[i] = (adv[i] - m) / den;
}

}  // namespace pulse

using namespace pulse;

extern "C" {

int pulse_policy_sample(const float* mu, int64_t mu_stride, const float* logstd, const float* noise, int64_t noise_stride, const float* value_raw, int64_t value_stride,
                        const double* value_mean, const double* value_var, int32_t rows, int32_t num_actions, float* actions, int64_t actions_stride, float* sigmas,
                        int64_t sigmas_stride, float* neglogp, int64_t neglogp_stride, float* values, int64_t values_out_stride, float* mus_out, int64_t mus_out_stride,
                        pulse_stream_t s) {
    PULSE_REQUIRE(rows >= 0 && num_actions >= 1, "pulse_policy_sample: bad sizes");
    if (rows == 0) return PULSE_OK;
    PULSE_REQUIRE(mu && logstd && noise && actions && neglogp, "pulse_policy_sample: null pointer");
    PULSE_REQUIRE(values == nullptr || value_raw != nullptr, "pulse_policy_sample: values requested without value_raw");
    PULSE_REQUIRE((value_mean == nullptr) == (value_var == nullptr), "pulse_policy_sample: value mean/var must come together");
    const long long threads = (long long)rows * kLanesPerSample;
    hipLaunchKernelGGL(policy_sample_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, as_stream(s), mu, (long long)mu_stride, logstd, noise,
                       (long long)noise_stride, value_raw, (long long)value_stride, value_mean, value_var, rows, num_actions, actions, (long long)actions_stride, sigmas,
                       (long long)sigmas_stride, neglogp, (long long)neglogp_stride, values, (long long)values_out_stride, mus_out, (long long)mus_out_stride);
    return check_launch("pulse_policy_sample");
}

int pulse_sizeof_ppo_loss_args(void) { return (int)sizeof(pulse_ppo_loss_args); }

int pulse_ppo_loss(const pulse_ppo_loss_args* args, pulse_stream_t s) {
    PULSE_REQUIRE(args != nullptr, "pulse_ppo_loss: null args");
    const pulse_ppo_loss_args& a = *args;
    PULSE_REQUIRE(a.rows >= 1 && a.num_actions >= 1 && a.num_blocks >= 1, "pulse_ppo_loss: bad sizes");
    PULSE_REQUIRE(a.mu && a.value && a.logstd && a.old_logstd && a.actions && a.old_mu && a.old_neglogp && a.advantages && a.returns &&
                      a.dmu && a.dvalue && a.partials, "pulse_ppo_loss: null pointer");
    PULSE_REQUIRE(!a.clip_value || a.old_values, "pulse_ppo_loss: clip_value needs old_values");
    const auto kernel = a.num_actions <= kLanesPerSample * kLossCols && gemm_option(8) == 0 ? ppo_loss_kernel<true> : ppo_loss_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(a.num_blocks), dim3(256), 0, as_stream(s), a);
    return check_launch("pulse_ppo_loss");
}

int pulse_advantage_moments(const float* returns, const float* values, int64_t count, float* adv, double* partials, int32_t num_blocks, pulse_stream_t s) {
    PULSE_REQUIRE(count >= 2 && num_blocks >= 1, "pulse_advantage_moments: need >= 2 samples");
    PULSE_REQUIRE(returns && values && adv && partials, "pulse_advantage_moments: null pointer");
    hipLaunchKernelGGL(adv_moments_kernel, dim3(num_blocks), dim3(256), 0, as_stream(s), returns, values, (long long)count, adv, partials);
    return check_launch("pulse_advantage_moments");
}

int pulse_advantage_normalize(float* adv, int64_t count, const double* partials, int32_t num_blocks, pulse_stream_t s) {
    PULSE_REQUIRE(count >= 2 && num_blocks >= 1 && adv && partials, "pulse_advantage_normalize: bad arguments");
    long long blocks = (count + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(adv_normalize_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(s), adv, (long long)count, partials, num_blocks);
    return check_launch("pulse_advantage_normalize");
}
}
