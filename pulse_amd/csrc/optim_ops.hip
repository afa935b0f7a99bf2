// The optimiser step of the PPO update on gfx950 (HBM-bound): sqnorm_partial / adam_step = clip_grad_norm_ + Adam.step over one flat parameter
// buffer (phc/learning/common_agent.py:472-478, :66).  Compiled with -ffp-contract=off.
#include "learner_math.h"

namespace pulse {

__global__ void __launch_bounds__(256) sqnorm_partial_kernel(const float* __restrict__ x, long long count, float* __restrict__ partials) {
    __shared__ float red[1][4];
    float s = 0.f;
    const long long n4 = count >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 v = x4[i];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    if (blockIdx.x == 0) for (long long i = (n4 << 2) + threadIdx.x; i < count; i += 256) s += x[i] * x[i];
    const float t = block_sum(s, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long long count, float lr,
                                          float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt, float max_norm, const float* __restrict__ sq_partials,
                                          int npart, float* __restrict__ norm_out) {
    __shared__ float red[1][4];
    __shared__ float s_coef;
    float coef = 1.0f;
    if (sq_partials) {
        double s = 0.0;
        for (int i = threadIdx.x; i < npart; i += 256) s += (double)sq_partials[i];
        const float t = block_sum(s, red);
        if (threadIdx.x == 0) {
            const float norm = sqrtf(t);
            if (norm_out && blockIdx.x == 0) *norm_out = norm;
            float c = 1.0f;
            if (max_norm > 0.f) c = fminf(max_norm / (norm + 1e-6f), 1.0f);   // clip_grad_norm_
            s_coef = c;
        }
        __syncthreads();
        coef = s_coef;
    }
    const float step_size = lr / bc1;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        float gi = g[i] * coef;
        const float pi = p[i];
        if (wd != 0.f) gi += wd * pi;
        const float mi = m[i] + (gi - m[i]) * (1.0f - b1);           // exp_avg.lerp_(grad, 1 - beta1)
        const float vi = v[i] * b2 + (1.0f - b2) * (gi * gi);        // exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2)
        m[i] = mi; v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = pi - step_size * (mi / denom);
    }
}

__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long long count,
                                                  float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt, float max_norm,
                                                  const float* __restrict__ sq_partials, int npart, float* __restrict__ norm_out) {
    adam_body(p, g, m, v, count, lr, b1, b2, eps, wd, bc1, bc2_sqrt, max_norm, sq_partials, npart, norm_out);
}

// the same step over up to four flat buffers in ONE launch (blockIdx.y = buffer): one optimiser over several parameter groups
// (AMPAgent: policy + discriminator, amp_agent.py:136-140) with the joint gradient-norm clip; per element exactly adam_kernel's arithmetic
struct AdamGroups { float* p[4]; const float* g[4]; float* m[4]; float* v[4]; long long count[4]; };
__global__ void __launch_bounds__(256) adam_multi_kernel(const AdamGroups a, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt, float max_norm,
                                                        const float* __restrict__ sq_partials, int npart, float* __restrict__ norm_out) {
    const int k = blockIdx.y;
    adam_body(a.p[k], a.g[k], a.m[k], a.v[k], a.count[k], lr, b1, b2, eps, wd, bc1, bc2_sqrt, max_norm, sq_partials, npart, k == 0 ? norm_out : nullptr);
}

}  // namespace pulse

using namespace pulse;

// what both Adam entries hand their kernel: the bias corrections (in double like torch's python floats, passed as fp32) and the grid over the longest buffer
struct AdamLaunch { float bc1, bc2_sqrt; unsigned blocks; };
static AdamLaunch adam_launch(float beta1, float beta2, int32_t step, long long most) {
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    return AdamLaunch{(float)bc1, (float)sqrt(bc2), (unsigned)(most > 2048LL * 256 ? 2048 : (most + 255) / 256)};
}

extern "C" {

int pulse_sqnorm_partial(const float* x, int64_t count, float* partials, int32_t num_blocks, pulse_stream_t s) {
    PULSE_REQUIRE(count >= 0 && num_blocks >= 1 && x && partials, "pulse_sqnorm_partial: bad arguments");
    PULSE_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0, "pulse_sqnorm_partial: x must be 16-byte aligned");
    hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(num_blocks), dim3(256), 0, as_stream(s), x, (long long)count, partials);
    return check_launch("pulse_sqnorm_partial");
}

int pulse_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t count, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int32_t step, float max_norm, const float* sqnorm_partials, int32_t num_partials, float* grad_norm_out, pulse_stream_t s) {
    PULSE_REQUIRE(count >= 0 && step >= 1, "pulse_adam_step: bad count / step");
    if (count == 0) return PULSE_OK;
    PULSE_REQUIRE(params && grads && exp_avg && exp_avg_sq, "pulse_adam_step: null pointer");
    PULSE_REQUIRE(sqnorm_partials == nullptr || num_partials >= 1, "pulse_adam_step: bad partial count");
    const AdamLaunch l = adam_launch(beta1, beta2, step, count);
    hipLaunchKernelGGL(adam_kernel, dim3(l.blocks), dim3(256), 0, as_stream(s), params, grads, exp_avg, exp_avg_sq, (long long)count, lr, beta1, beta2, eps, weight_decay,
                       l.bc1, l.bc2_sqrt, max_norm, sqnorm_partials, num_partials, grad_norm_out);
    return check_launch("pulse_adam_step");
}

int pulse_adam_step_multi(int32_t num_groups, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const int64_t* counts,
                          float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, float max_norm, const float* sqnorm_partials,
                          int32_t num_partials, float* grad_norm_out, pulse_stream_t s) {
    PULSE_REQUIRE(num_groups >= 1 && num_groups <= 4 && step >= 1, "pulse_adam_step_multi: 1..4 groups, step >= 1");
    PULSE_REQUIRE(params && grads && exp_avg && exp_avg_sq && counts, "pulse_adam_step_multi: null pointer");
    PULSE_REQUIRE(sqnorm_partials == nullptr || num_partials >= 1, "pulse_adam_step_multi: bad partial count");
    AdamGroups a;
    long long most = 0;
    for (int k = 0; k < 4; ++k) {
        const bool on = k < num_groups;
        a.p[k] = on ? params[k] : nullptr; a.g[k] = on ? grads[k] : nullptr; a.m[k] = on ? exp_avg[k] : nullptr; a.v[k] = on ? exp_avg_sq[k] : nullptr;
        a.count[k] = on ? counts[k] : 0;
        PULSE_REQUIRE(!on || (counts[k] >= 0 && (counts[k] == 0 || (params[k] && grads[k] && exp_avg[k] && exp_avg_sq[k]))), "pulse_adam_step_multi: bad group");
        if (a.count[k] > most) most = a.count[k];
    }
    if (most == 0) return PULSE_OK;
    const AdamLaunch l = adam_launch(beta1, beta2, step, most);
    hipLaunchKernelGGL(adam_multi_kernel, dim3(l.blocks, (unsigned)num_groups), dim3(256), 0, as_stream(s), a, lr, beta1, beta2, eps, weight_decay, l.bc1, l.bc2_sqrt,
                       max_norm, sqnorm_partials, num_partials, grad_norm_out);
    return check_launch("pulse_adam_step_multi");
}
}
