// PULSE VAE head algebra in three launches (no autograd tape on the product path).
//
// Replaces the tensor-op chains (and their autograd backward) of
//   AMPZBuilder.Network.form_embedding        phc/learning/amp_network_z_builder.py:79-121   (logvar clamp, re-parameterisation)
//   AMPAgent._optimize_kin                    phc/learning/amp_agent.py:771-849             (action RMSE, KL vs the learned prior,
//                                                                                            AR(1) latent smoothness with seam mask, regulariser)
//   kl_multi                                  phc/learning/loss_functions.py:3-10
// One 32-lane half-wave per minibatch row (lane = latent dimension, embedding_size <= 32), 8 rows per 256-thread workgroup; row
// reductions are 32-lane butterflies, loss sums go through per-workgroup partials that the host-side sum reduces in a fixed order
// (deterministic).  Compiled with -ffp-contract=off: the expressions are written in the reference's operation order.
//
// Prior / posterior variants (amp_network_z_builder.py:118-119, 226-241; amp_agent.py:785-789; torch_utils.py:38-43) are template
// parameters, so the shipped form (learned prior, Gaussian posterior) is the instantiation it always was:
//   PRIOR   learned [mu | logvar] heads / fixed: mu heads (E wide) and a constant, unclamped log-variance / none: KL against N(0, I)
//   SPRIOR  the fixed prior's mean goes through project_to_norm(., embedding_norm) first
//   SPOST   z is projected after the re-parameterisation; the heads themselves (KL, AR(1), regulariser) stay unprojected
// A fourth launch, pulse_vae_embed_prior, is the generation step: z drawn from the prior instead of the posterior (:101-119).
#include "common.h"

namespace pulse {

constexpr int kVL = 32;   // lanes per row

__device__ __forceinline__ float vclamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

constexpr int kLearned = PULSE_VAE_PRIOR_LEARNED, kFixed = PULSE_VAE_PRIOR_FIXED, kNone = PULSE_VAE_PRIOR_NONE;

// project_to_norm(x, norm, "sphere") = x / (||x|| / norm + 1e-8) over one row (torch_utils.py:38-43).  Every lane of the half-wave calls
// these; an idle lane (lane >= embedding_size) passes zeros.
__device__ __forceinline__ float sphere_project(float v, float norm) { return v / (sqrtf(lane_sum<kVL>(v * v)) / norm + 1e-8f); }
// g = d loss / d project(v) -> d loss / d v = g / s - v (g . v) / (s^2 norm ||v||), s = ||v|| / norm + 1e-8; the second term is absent
// at ||v|| = 0 (torch.norm's sub-gradient)
__device__ __forceinline__ float sphere_backward(float g, float v, float norm) {
    const float n = sqrtf(lane_sum<kVL>(v * v)), s = n / norm + 1e-8f, gv = lane_sum<kVL>(g * v);
    float o = g / s;
    if (n > 0.f) o -= v * gv / (s * s * norm * n);
    return o;
}

// ---- form_embedding: z = mu + exp(0.5 clamp(logvar)) eps, written with the self observation into the decoder's (and the critic's)
// concat buffer.  eps == NULL: z = mu (flags.test, amp_network_z_builder.py:94-95).  SPOST: z / (||z|| / embedding_norm + 1e-8) is what
// is written (:118-119, after the flags.test replacement); the row norm needs the whole row first, so the z columns go half-wave per row.
template <bool SPOST>
__global__ void __launch_bounds__(256) vae_embed_kernel(const pulse_vae_embed_args a) {
    const int E = a.embedding_size, S = a.self_obs_size;
    if (!SPOST) {
        const long long total = (long long)a.rows * (S + E);
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
            const int r = (int)(i / (S + E)), c = (int)(i - (long long)r * (S + E));
            if (c < S) {
                const float v = a.x[(long long)r * a.x_stride + c];
                a.ain[(long long)r * a.ain_stride + c] = v;
                if (a.cin) a.cin[(long long)r * a.cin_stride + c] = v;
            } else {
                const int e = c - S;
                const float* h = a.heads + (long long)r * a.heads_stride;
                const float mu = h[e];
                float lv = h[E + e];
                if (a.clamp_logvar) lv = vclamp(lv, -5.0f, a.clamp_max);
                const float z = a.eps ? mu + expf(0.5f * lv) * a.eps[(long long)r * a.eps_stride + e] : mu;
                a.ain[(long long)r * a.ain_stride + a.z_col + e] = z;
            }
        }
    } else {
        const long long total = (long long)a.rows * S;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
            const long long r = i / S;
            const int c = (int)(i - r * S);
            const float v = a.x[r * a.x_stride + c];
            a.ain[r * a.ain_stride + c] = v;
            if (a.cin) a.cin[r * a.cin_stride + c] = v;
        }
        const int slot = threadIdx.x / kVL, l = threadIdx.x % kVL;
        for (long long base = (long long)blockIdx.x * 8; base < a.rows; base += (long long)gridDim.x * 8) {
            const long long r = base + slot;
            if (r >= a.rows) continue;
            float z = 0.f;
            if (l < E) {
                const float* h = a.heads + r * a.heads_stride;
                const float mu = h[l];
                float lv = h[E + l];
                if (a.clamp_logvar) lv = vclamp(lv, -5.0f, a.clamp_max);
                z = a.eps ? mu + expf(0.5f * lv) * a.eps[r * a.eps_stride + l] : mu;
            }
            z = sphere_project(z, a.embedding_norm);
            if (l < E) a.ain[r * a.ain_stride + a.z_col + l] = z;
        }
    }
}

// ---- form_embedding under flags.debug (amp_network_z_builder.py:101-119): z is drawn from the PRIOR, the encoder heads are not read.
//   kLearned / kFixed  z = prior_mu + eps * exp(0.5 prior_logvar) with (prior_mu, prior_logvar) as compute_prior returns them (:226-248):
//                      learned heads [mu | logvar], the log-variance clamped; fixed heads = the mean (projected when SPRIOR) and the constant,
//                      unclamped log-variance.  logvar_override replaces the log-variance by a constant (the commented variants of :110-111);
//                      eps == NULL: z = prior_mu (:109)
//   kNone              z = eps (:116)
// SPOST projects z afterwards (:118-119).  Half-wave per row whatever the mode; the self-observation columns are copied element-wise.
template <int PRIOR, bool SPRIOR, bool SPOST>
__global__ void __launch_bounds__(256) vae_embed_prior_kernel(const pulse_vae_embed_prior_args a) {
    const int E = a.embedding_size, S = a.self_obs_size;
    const long long total = (long long)a.rows * S;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / S;
        const int c = (int)(i - r * S);
        const float v = a.x[r * a.x_stride + c];
        a.ain[r * a.ain_stride + c] = v;
        if (a.cin) a.cin[r * a.cin_stride + c] = v;
    }
    const int slot = threadIdx.x / kVL, l = threadIdx.x % kVL;
    for (long long base = (long long)blockIdx.x * 8; base < a.rows; base += (long long)gridDim.x * 8) {
        const long long r = base + slot;
        if (r >= a.rows) continue;
        const bool on = l < E;
        float z = 0.f;
        if (PRIOR == kNone) {
            if (on) z = a.eps[r * a.eps_stride + l];
        } else {
            float mu = on ? a.pheads[r * a.pheads_stride + l] : 0.f;
            if (SPRIOR) mu = sphere_project(mu, a.embedding_norm);
            z = mu;
            if (on && a.eps) {
                float lv;
                if (a.logvar_override) lv = a.logvar_override_value;
                else if (PRIOR == kFixed) lv = a.prior_fixed_logvar;
                else {
                    lv = a.pheads[r * a.pheads_stride + E + l];
                    if (a.clamp_logvar) lv = vclamp(lv, -5.0f, a.clamp_max);
                }
                z = mu + a.eps[r * a.eps_stride + l] * expf(0.5f * lv);
            }
        }
        if (SPOST) z = sphere_project(z, a.embedding_norm);
        if (on) {
            a.ain[r * a.ain_stride + a.z_col + l] = z;
            if (a.z_out) a.z_out[r * a.z_out_stride + l] = z;
        }
    }
}

// ---- HumanoidZ.compute_z_actions under the sphere posterior (humanoid_z.py:101-107): out = project_to_norm(a [+ b], norm), one
// half-wave per row.
__global__ void __launch_bounds__(256) vae_project_kernel(const float* a, long long a_stride, const float* b, long long b_stride, float* out,
                                                          long long out_stride, int rows, int cols, float norm) {
    const int slot = threadIdx.x / kVL, l = threadIdx.x % kVL;
    for (long long base = (long long)blockIdx.x * 8; base < rows; base += (long long)gridDim.x * 8) {
        const long long r = base + slot;
        if (r >= rows) continue;
        float v = 0.f;
        if (l < cols) v = b ? b[r * b_stride + l] + a[r * a_stride + l] : a[r * a_stride + l];
        v = sphere_project(v, norm);
        if (l < cols) out[r * out_stride + l] = v;
    }
}

// keep-mask of AR(1) error row (sequence s, step i -> i + 1): consecutive progress values and neither step within the first frames
__device__ __forceinline__ bool ar1_keep(const int64_t* prog, long long r0) {
    const long long p0 = (long long)prog[r0], p1 = (long long)prog[r0 + 1];
    return (p1 - p0) == 1 && !(p0 <= 2 || p1 <= 2);
}

// ---- losses of _optimize_kin + d loss / d pred_action.  partials[block][8] = sums over the block's rows of
//   [0] ||pred - gt||   [1] kl_multi row   [2] ||masked AR(1) error||   [3] prior_mu^2   [4] vae_mu^2   [5] prior_logvar^2   [6] vae_logvar^2
// kFixed: the prior heads are the mean alone (projected when SPRIOR), the log-variance is the constant prior_fixed_logvar -- not clamped
// (:237-241), and its square still counts in [5].  kNone: [1] is the row of -0.5 sum(1 + logvar - mu^2 - exp(logvar)) (amp_agent.py:789).
template <int PRIOR, bool SPRIOR>
__global__ void __launch_bounds__(256) vae_kin_loss_kernel(const pulse_vae_kin_args a) {
    __shared__ float red[8][8];
    const int slot = threadIdx.x / kVL, l = threadIdx.x % kVL;
    const int E = a.embedding_size, A = a.num_actions, T = a.horizon;
    const float inv_rows = 1.0f / (float)a.rows;
    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long long base = (long long)blockIdx.x * 8; base < a.rows; base += (long long)gridDim.x * 8) {
        const long long i = base + slot;
        if (i >= a.rows) continue;
        // action loss: torch.norm(pred - gt, dim=-1).mean()
        const float* pr = a.pred + i * a.pred_stride;
        const float* gt = a.gt + i * a.gt_stride;
        float sq = 0.f;
        for (int j = l; j < A; j += kVL) { const float d = pr[j] - gt[j]; sq += d * d; }
        const float nrm = sqrtf(lane_sum<kVL>(sq));
        float* dmu = a.dmu + i * a.dmu_stride;
        for (int j = l; j < A; j += kVL) dmu[j] = nrm > 0.f ? ((pr[j] - gt[j]) / nrm) * inv_rows : 0.f;
        // KL(q || prior), loss_functions.py:3-10; against N(0, I) without a prior
        float kl = 0.f, e_pm = 0.f, e_qm = 0.f, e_pv = 0.f, e_qv = 0.f, err2 = 0.f;
        const float* zh = a.zheads + i * a.zheads_stride;
        float pm_s = 0.f;
        if (PRIOR == kFixed && SPRIOR) pm_s = sphere_project(l < E ? a.pheads[i * a.pheads_stride + l] : 0.f, a.embedding_norm);
        if (l < E) {
            const float* ph = a.pheads + i * a.pheads_stride;
            const float qm = zh[l], pm = PRIOR == kNone ? 0.f : SPRIOR ? pm_s : ph[l];
            float qv = zh[E + l], pv = PRIOR == kLearned ? ph[E + l] : PRIOR == kFixed ? a.prior_fixed_logvar : 0.f;
            if (a.clamp_logvar) { qv = vclamp(qv, -5.0f, a.clamp_max); if (PRIOR == kLearned) pv = vclamp(pv, -5.0f, a.clamp_max); }
            if (PRIOR != kNone) {
                const float ep = expf(pv);
                const float dm = qm - pm;
                kl = 0.5f * (pv - qv + expf(qv) / ep + (dm * dm) / ep - 1.0f);
            } else {
                kl = -0.5f * (1.0f + qv - qm * qm - expf(qv));
            }
            e_pm = pm * pm; e_qm = qm * qm; e_pv = pv * pv; e_qv = qv * qv;
            // AR(1) error row (i -> i + 1) of this sequence, amp_agent.py:792-808
            if (a.use_ar1 && (i % T) < T - 1 && ar1_keep(a.progress, i)) {
                const float er = zh[a.zheads_stride + l] - qm * 0.99f;
                err2 = er * er;
            }
        }
        kl = lane_sum<kVL>(kl);
        const float ar = a.use_ar1 ? sqrtf(lane_sum<kVL>(err2)) : 0.f;
        if (a.use_regu) { e_pm = lane_sum<kVL>(e_pm); e_qm = lane_sum<kVL>(e_qm); e_pv = lane_sum<kVL>(e_pv); e_qv = lane_sum<kVL>(e_qv); }
        acc[0] += nrm; acc[1] += kl; acc[2] += ar; acc[3] += e_pm; acc[4] += e_qm; acc[5] += e_pv; acc[6] += e_qv;
    }
    if (l == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) red[k][slot] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += red[threadIdx.x][k];
        a.partials[(long long)blockIdx.x * 8 + threadIdx.x] = s;
    }
    if (threadIdx.x == 7) a.partials[(long long)blockIdx.x * 8 + 7] = 0.f;
}

// ---- head backward: d loss / d (encoder heads) and d loss / d (prior heads) from the decoder's dz (re-parameterisation), the KL term,
// the AR(1) term and the regulariser.  Coefficients arrive with the batch means folded in.  SPOST: dz is the gradient of the PROJECTED
// latent; z is recomputed from the heads and eps and dz goes through the projection's Jacobian first.  kFixed: dpheads is E wide (the
// mean alone; through the projection's Jacobian when SPRIOR), the constant log-variance gets nothing.  kNone: the KL pulls towards N(0, I).
template <int PRIOR, bool SPRIOR, bool SPOST>
__global__ void __launch_bounds__(256) vae_head_backward_kernel(const pulse_vae_head_bwd_args a) {
    const int slot = threadIdx.x / kVL, l = threadIdx.x % kVL;
    const int E = a.embedding_size, T = a.horizon;
    for (long long base = (long long)blockIdx.x * 8; base < a.rows; base += (long long)gridDim.x * 8) {
        const long long i = base + slot;
        if (i >= a.rows) continue;
        const float* zh = a.zheads + i * a.zheads_stride;
        const bool on = l < E;
        float qm = 0.f, qv_raw = 0.f, qv = 0.f;
        bool in_q = true;
        if (on) {
            qm = zh[l]; qv_raw = zh[E + l]; qv = qv_raw;
            if (a.clamp_logvar) { qv = vclamp(qv_raw, -5.0f, a.clamp_max); in_q = qv_raw >= -5.0f && qv_raw <= a.clamp_max; }
        }
        float g_qm = 0.f, g_qv = 0.f;
        if (!SPOST) {
            if (on && a.dz) {                                       // z = mu + exp(0.5 logvar) eps
                const float dz = a.dz[i * a.dz_stride + l];
                g_qm = dz;
                if (a.eps) g_qv = dz * (0.5f * expf(0.5f * qv) * a.eps[i * a.eps_stride + l]);
            }
        } else if (a.dz) {                                          // z' = project(z): the whole half-wave takes part in the row sums
            float z = 0.f, dz = 0.f, dz_dqv = 0.f;
            if (on) {
                dz = a.dz[i * a.dz_stride + l];
                z = qm;
                if (a.eps) {
                    const float sd = expf(0.5f * qv), e = a.eps[i * a.eps_stride + l];
                    z = qm + sd * e;
                    dz_dqv = 0.5f * sd * e;
                }
            }
            const float gz = sphere_backward(dz, z, a.embedding_norm);
            if (on) { g_qm = gz; g_qv = gz * dz_dqv; }
        }
        if (PRIOR == kLearned && a.pheads) {
            const float* ph = a.pheads + i * a.pheads_stride;
            float g_pm = 0.f, g_pv = 0.f;
            if (on) {
                const float pm = ph[l], pv_raw = ph[E + l];
                float pv = pv_raw;
                bool in_p = true;
                if (a.clamp_logvar) { pv = vclamp(pv_raw, -5.0f, a.clamp_max); in_p = pv_raw >= -5.0f && pv_raw <= a.clamp_max; }
                const float ep = expf(pv), dm = qm - pm, rq = expf(qv) / ep;
                g_qm += a.c_kl * (dm / ep);
                g_qv += a.c_kl * (0.5f * (rq - 1.0f));
                g_pm = -a.c_kl * (dm / ep) + a.c_regu * 2.0f * pm;
                g_pv = in_p ? a.c_kl * (0.5f * (1.0f - rq - (dm * dm) / ep)) + a.c_regu * 2.0f * pv : 0.f;
                g_qm += a.c_regu * 2.0f * qm;
                g_qv += a.c_regu * 2.0f * qv;
            }
            if (on && a.dpheads) {
                float* o = a.dpheads + i * a.dpheads_stride;
                o[l] = g_pm; o[E + l] = g_pv;
            }
        }
        if (PRIOR == kFixed && a.pheads) {
            const float raw = on ? a.pheads[i * a.pheads_stride + l] : 0.f;
            const float pm = SPRIOR ? sphere_project(raw, a.embedding_norm) : raw;
            float g_pm = 0.f;
            if (on) {
                const float ep = expf(a.prior_fixed_logvar), dm = qm - pm, rq = expf(qv) / ep;
                g_qm += a.c_kl * (dm / ep);
                g_qv += a.c_kl * (0.5f * (rq - 1.0f));
                g_pm = -a.c_kl * (dm / ep) + a.c_regu * 2.0f * pm;
                g_qm += a.c_regu * 2.0f * qm;
                g_qv += a.c_regu * 2.0f * qv;
            }
            if (SPRIOR) g_pm = sphere_backward(g_pm, raw, a.embedding_norm);
            if (on && a.dpheads) a.dpheads[i * a.dpheads_stride + l] = g_pm;
        }
        if (PRIOR == kNone && on && a.c_kl != 0.f) {                // d / d (mu, logvar) of -0.5 (1 + logvar - mu^2 - exp(logvar))
            g_qm += a.c_kl * qm;
            g_qv += a.c_kl * (0.5f * (expf(qv) - 1.0f));
        }
        if (a.c_ar1 != 0.f) {
            // error rows touching this step: (i - 1 -> i) contributes + err / ||err||, (i -> i + 1) contributes - 0.99 err / ||err||
            const int ti = (int)(i % T);
            float e_prev = 0.f, e_next = 0.f;
            const bool has_prev = ti > 0 && ar1_keep(a.progress, i - 1), has_next = ti < T - 1 && ar1_keep(a.progress, i);
            if (on && has_prev) e_prev = qm - zh[l - a.zheads_stride] * 0.99f;
            if (on && has_next) e_next = zh[a.zheads_stride + l] - qm * 0.99f;
            const float n_prev = sqrtf(lane_sum<kVL>(e_prev * e_prev)), n_next = sqrtf(lane_sum<kVL>(e_next * e_next));
            if (on) {
                if (n_prev > 0.f) g_qm += a.c_ar1 * (e_prev / n_prev);
                if (n_next > 0.f) g_qm += a.c_ar1 * (-0.99f * (e_next / n_next));
            }
        }
        if (on) {
            float* o = a.dzheads + i * a.dzheads_stride;
            o[l] = g_qm;
            o[E + l] = in_q ? g_qv : 0.f;
        }
    }
}

}  // namespace pulse

using namespace pulse;

// the widths of the prior heads per mode: [mu | logvar] learned, mu alone fixed
static inline int prior_width(int mode, int E) { return mode == kLearned ? 2 * E : E; }

template <int PRIOR, bool SPRIOR>
static void launch_head_backward(const pulse_vae_head_bwd_args& a, dim3 grid, pulse_stream_t s) {
    if (a.sphere_posterior) hipLaunchKernelGGL((vae_head_backward_kernel<PRIOR, SPRIOR, true>), grid, dim3(256), 0, as_stream(s), a);
    else hipLaunchKernelGGL((vae_head_backward_kernel<PRIOR, SPRIOR, false>), grid, dim3(256), 0, as_stream(s), a);
}

template <int PRIOR, bool SPRIOR>
static void launch_embed_prior(const pulse_vae_embed_prior_args& a, dim3 grid, pulse_stream_t s) {
    if (a.sphere_posterior) hipLaunchKernelGGL((vae_embed_prior_kernel<PRIOR, SPRIOR, true>), grid, dim3(256), 0, as_stream(s), a);
    else hipLaunchKernelGGL((vae_embed_prior_kernel<PRIOR, SPRIOR, false>), grid, dim3(256), 0, as_stream(s), a);
}

extern "C" {

int pulse_sizeof_vae_embed_prior_args(void) { return (int)sizeof(pulse_vae_embed_prior_args); }

int pulse_vae_embed_prior(const pulse_vae_embed_prior_args* args, pulse_stream_t s) {
    PULSE_REQUIRE(args != nullptr, "pulse_vae_embed_prior: null args");
    const pulse_vae_embed_prior_args& a = *args;
    if (a.rows == 0) return PULSE_OK;
    PULSE_REQUIRE(a.rows > 0 && a.embedding_size >= 1 && a.embedding_size <= kVL && a.self_obs_size >= 0,
                  "pulse_vae_embed_prior: bad sizes (embedding_size <= 32)");
    PULSE_REQUIRE(a.prior_mode == kLearned || a.prior_mode == kFixed || a.prior_mode == kNone, "pulse_vae_embed_prior: unknown prior_mode");
    PULSE_REQUIRE(a.x && a.ain, "pulse_vae_embed_prior: null pointer");
    PULSE_REQUIRE(a.x_stride >= a.self_obs_size && a.ain_stride >= (int64_t)a.z_col + a.embedding_size && a.z_col >= a.self_obs_size,
                  "pulse_vae_embed_prior: strides / column offsets do not cover the rows");
    PULSE_REQUIRE(a.prior_mode == kNone || a.pheads, "pulse_vae_embed_prior: a learned / fixed prior needs the prior heads");
    PULSE_REQUIRE(a.prior_mode == kNone || a.pheads_stride >= prior_width(a.prior_mode, a.embedding_size),
                  "pulse_vae_embed_prior: pheads_stride too small (2E learned, E fixed)");
    PULSE_REQUIRE(a.prior_mode != kNone || a.eps, "pulse_vae_embed_prior: without a prior z is the noise itself: eps must be given");
    PULSE_REQUIRE(!a.eps || a.eps_stride >= a.embedding_size, "pulse_vae_embed_prior: eps_stride too small");
    PULSE_REQUIRE(!a.cin || a.cin_stride >= a.self_obs_size, "pulse_vae_embed_prior: cin_stride too small");
    PULSE_REQUIRE(!a.z_out || a.z_out_stride >= a.embedding_size, "pulse_vae_embed_prior: z_out_stride too small");
    const bool sprior = a.prior_mode == kFixed && a.sphere_prior;       // acts under the fixed prior only (amp_network_z_builder.py:237-239)
    PULSE_REQUIRE(!(sprior || a.sphere_posterior) || a.embedding_norm > 0.f, "pulse_vae_embed_prior: the sphere projections need embedding_norm > 0");
    long long blocks = ((long long)a.rows * a.self_obs_size + 255) / 256, row_blocks = ((long long)a.rows + 7) / 8;
    if (blocks < row_blocks) blocks = row_blocks;
    if (blocks > 4096) blocks = 4096;
    const dim3 grid((unsigned)blocks);
    if (a.prior_mode == kLearned) launch_embed_prior<kLearned, false>(a, grid, s);
    else if (a.prior_mode == kNone) launch_embed_prior<kNone, false>(a, grid, s);
    else if (sprior) launch_embed_prior<kFixed, true>(a, grid, s);
    else launch_embed_prior<kFixed, false>(a, grid, s);
    return check_launch("pulse_vae_embed_prior");
}

int pulse_sizeof_vae_embed_args(void) { return (int)sizeof(pulse_vae_embed_args); }
int pulse_sizeof_vae_kin_args(void) { return (int)sizeof(pulse_vae_kin_args); }
int pulse_sizeof_vae_head_bwd_args(void) { return (int)sizeof(pulse_vae_head_bwd_args); }

int pulse_vae_embed(const pulse_vae_embed_args* args, pulse_stream_t s) {
    PULSE_REQUIRE(args != nullptr, "pulse_vae_embed: null args");
    const pulse_vae_embed_args& a = *args;
    if (a.rows == 0) return PULSE_OK;
    PULSE_REQUIRE(a.rows > 0 && a.embedding_size >= 1 && a.self_obs_size >= 0, "pulse_vae_embed: bad sizes");
    PULSE_REQUIRE(a.heads && a.x && a.ain, "pulse_vae_embed: null pointer");
    PULSE_REQUIRE(a.heads_stride >= 2 * a.embedding_size && a.x_stride >= a.self_obs_size && a.ain_stride >= a.z_col + a.embedding_size &&
                  a.z_col >= a.self_obs_size, "pulse_vae_embed: strides / column offsets do not cover the rows");
    PULSE_REQUIRE(!a.eps || a.eps_stride >= a.embedding_size, "pulse_vae_embed: eps_stride too small");
    PULSE_REQUIRE(!a.cin || a.cin_stride >= a.self_obs_size, "pulse_vae_embed: cin_stride too small");
    if (!a.sphere_posterior) {
        long long blocks = ((long long)a.rows * (a.self_obs_size + a.embedding_size) + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(vae_embed_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, as_stream(s), a);
    } else {
        PULSE_REQUIRE(a.embedding_size <= kVL && a.embedding_norm > 0.f, "pulse_vae_embed: the sphere posterior needs embedding_size <= 32 and embedding_norm > 0");
        long long blocks = ((long long)a.rows * a.self_obs_size + 255) / 256, row_blocks = ((long long)a.rows + 7) / 8;
        if (blocks < row_blocks) blocks = row_blocks;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(vae_embed_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, as_stream(s), a);
    }
    return check_launch("pulse_vae_embed");
}

int pulse_vae_project(const float* a, int64_t a_stride, const float* b, int64_t b_stride, float* out, int64_t out_stride, int32_t rows, int32_t cols,
                      float norm, pulse_stream_t s) {
    if (rows == 0) return PULSE_OK;
    PULSE_REQUIRE(rows > 0 && cols >= 1 && cols <= kVL && norm > 0.f, "pulse_vae_project: bad sizes (cols <= 32, norm > 0)");
    PULSE_REQUIRE(a && out, "pulse_vae_project: null pointer");
    PULSE_REQUIRE(a_stride >= cols && out_stride >= cols && (!b || b_stride >= cols), "pulse_vae_project: strides too small");
    long long blocks = ((long long)rows + 7) / 8;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(vae_project_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(s), a, (long long)a_stride, b, (long long)b_stride, out,
                       (long long)out_stride, (int)rows, (int)cols, norm);
    return check_launch("pulse_vae_project");
}

int pulse_vae_kin_loss(const pulse_vae_kin_args* args, pulse_stream_t s) {
    PULSE_REQUIRE(args != nullptr, "pulse_vae_kin_loss: null args");
    const pulse_vae_kin_args& a = *args;
    PULSE_REQUIRE(a.rows >= 1 && a.num_actions >= 1 && a.embedding_size >= 1 && a.embedding_size <= kVL && a.num_blocks >= 1, "pulse_vae_kin_loss: bad sizes (embedding_size <= 32)");
    PULSE_REQUIRE(a.prior_mode == kLearned || a.prior_mode == kFixed || a.prior_mode == kNone, "pulse_vae_kin_loss: unknown prior_mode");
    PULSE_REQUIRE(a.pred && a.gt && a.zheads && a.dmu && a.partials, "pulse_vae_kin_loss: null pointer");
    PULSE_REQUIRE(a.prior_mode == kNone || a.pheads, "pulse_vae_kin_loss: a learned / fixed prior needs the prior heads");
    PULSE_REQUIRE(a.prior_mode != kNone || !a.use_regu, "pulse_vae_kin_loss: the regulariser is undefined without a prior (amp_agent.py:810-813)");
    PULSE_REQUIRE(!a.use_ar1 || (a.progress && a.horizon >= 2 && a.rows % a.horizon == 0), "pulse_vae_kin_loss: the AR(1) term needs progress and rows = sequences x horizon");
    PULSE_REQUIRE(a.zheads_stride >= 2 * a.embedding_size && (a.prior_mode == kNone || a.pheads_stride >= prior_width(a.prior_mode, a.embedding_size)),
                  "pulse_vae_kin_loss: head strides too small");
    const bool sprior = a.prior_mode == kFixed && a.sphere_prior;       // the switch acts under the fixed prior only (amp_network_z_builder.py:237-239)
    PULSE_REQUIRE(!sprior || a.embedding_norm > 0.f, "pulse_vae_kin_loss: the sphere prior needs embedding_norm > 0");
    const dim3 grid((unsigned)a.num_blocks), block(256);
    if (a.prior_mode == kLearned) hipLaunchKernelGGL((vae_kin_loss_kernel<kLearned, false>), grid, block, 0, as_stream(s), a);
    else if (a.prior_mode == kNone) hipLaunchKernelGGL((vae_kin_loss_kernel<kNone, false>), grid, block, 0, as_stream(s), a);
    else if (sprior) hipLaunchKernelGGL((vae_kin_loss_kernel<kFixed, true>), grid, block, 0, as_stream(s), a);
    else hipLaunchKernelGGL((vae_kin_loss_kernel<kFixed, false>), grid, block, 0, as_stream(s), a);
    return check_launch("pulse_vae_kin_loss");
}

int pulse_vae_head_backward(const pulse_vae_head_bwd_args* args, pulse_stream_t s) {
    PULSE_REQUIRE(args != nullptr, "pulse_vae_head_backward: null args");
    const pulse_vae_head_bwd_args& a = *args;
    if (a.rows == 0) return PULSE_OK;
    PULSE_REQUIRE(a.rows > 0 && a.embedding_size >= 1 && a.embedding_size <= kVL, "pulse_vae_head_backward: bad sizes (embedding_size <= 32)");
    PULSE_REQUIRE(a.prior_mode == kLearned || a.prior_mode == kFixed || a.prior_mode == kNone, "pulse_vae_head_backward: unknown prior_mode");
    PULSE_REQUIRE(a.zheads && a.dzheads, "pulse_vae_head_backward: null pointer");
    PULSE_REQUIRE(a.zheads_stride >= 2 * a.embedding_size && a.dzheads_stride >= 2 * a.embedding_size, "pulse_vae_head_backward: head strides too small");
    const int pw = prior_width(a.prior_mode, a.embedding_size);
    PULSE_REQUIRE(!a.pheads || a.prior_mode == kNone || (a.pheads_stride >= pw && (!a.dpheads || a.dpheads_stride >= pw)), "pulse_vae_head_backward: prior strides too small");
    PULSE_REQUIRE(a.pheads || a.prior_mode == kNone || (a.c_kl == 0.f && a.c_regu == 0.f), "pulse_vae_head_backward: KL / regulariser terms need the prior heads");
    PULSE_REQUIRE(a.prior_mode != kNone || a.c_regu == 0.f, "pulse_vae_head_backward: the regulariser is undefined without a prior (amp_agent.py:810-813)");
    PULSE_REQUIRE(a.c_ar1 == 0.f || (a.progress && a.horizon >= 2 && a.rows % a.horizon == 0), "pulse_vae_head_backward: the AR(1) term needs progress and rows = sequences x horizon");
    PULSE_REQUIRE(!a.dz || a.dz_stride >= a.embedding_size, "pulse_vae_head_backward: dz_stride too small");
    PULSE_REQUIRE(!a.eps || a.eps_stride >= a.embedding_size, "pulse_vae_head_backward: eps_stride too small");
    const bool sprior = a.prior_mode == kFixed && a.sphere_prior;
    PULSE_REQUIRE(!(sprior || a.sphere_posterior) || a.embedding_norm > 0.f, "pulse_vae_head_backward: the sphere projections need embedding_norm > 0");
    long long blocks = ((long long)a.rows + 7) / 8;
    if (blocks > 4096) blocks = 4096;
    const dim3 grid((unsigned)blocks);
    if (a.prior_mode == kLearned) launch_head_backward<kLearned, false>(a, grid, s);
    else if (a.prior_mode == kNone) launch_head_backward<kNone, false>(a, grid, s);
    else if (sprior) launch_head_backward<kFixed, true>(a, grid, s);
    else launch_head_backward<kFixed, false>(a, grid, s);
    return check_launch("pulse_vae_head_backward");
}
}
