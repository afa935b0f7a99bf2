// The MCP composer stage of PHC (phc_kp_mcp_iccv.yaml / im_mcp.yaml): the policy's action is a weight vector over num_prim frozen PNN
// primitives.
//
// Replaces the tensor-op chains of
//   HumanoidImMCP.step                        phc/env/tasks/humanoid_im_mcp.py:56-67          (argmax + one_hot, weights[:, :, None] * x_all, sum)
//   AMPMCPBuilder.Network.__init__/eval_actor phc/learning/amp_network_mcp_builder.py:41-55, 64-86  (nn.Softmax(dim=1) behind the composer's last
//                                                                                              activation; mu = the composer's output)
// and the autograd backward of that tail (softmax, then the last layer's activation), which learning/graph.py cannot fuse into a next layer's
// input-gradient GEMM because the composer's last layer has no next layer.
// num_prim <= 32.  One thread per output element (compose) or per row (head).  Compiled with -ffp-contract=off: every product is rounded to
// fp32 before it is added, sums run with k ascending like torch.sum over dim 1.
#include <math.h>

#include "common.h"

namespace pulse {

constexpr int kMcpMaxPrim = 32;

struct McpComposeArgs {
    const float* w; long long w_stride;
    const float* x; long long x_stride; int a_pitch;
    float* out; long long out_stride;
    int rows, P, A, discrete;
};

// index of the first maximum of a weight row (torch.argmax: a NaN counts as the maximum)
__device__ __forceinline__ int mcp_argmax(const float* w, int P) {
    int best = 0;
    float bv = w[0];
    for (int k = 1; k < P; ++k) {
        const float v = w[k];
        if (bv == bv && (v > bv || v != v)) { bv = v; best = k; }
    }
    return best;
}

__global__ void __launch_bounds__(256) mcp_compose_kernel(const McpComposeArgs a) {
    const long long total = (long long)a.rows * a.A;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long e = i / a.A;
        const int c = (int)(i - e * a.A);
        const float* w = a.w + e * a.w_stride;
        const float* x = a.x + e * a.x_stride + c;
        const int hot = a.discrete ? mcp_argmax(w, a.P) : -1;       // one_hot(argmax).float(): the row becomes 0 / 1 and goes through the same sum
        float acc = (a.discrete ? (hot == 0 ? 1.f : 0.f) : w[0]) * x[0];
        for (int k = 1; k < a.P; ++k) {
            const float wk = a.discrete ? (hot == k ? 1.f : 0.f) : w[k];
            acc = acc + wk * x[(long long)k * a.a_pitch];
        }
        a.out[e * a.out_stride + c] = acc;
    }
}

struct McpHeadFwdArgs {
    const float* h; long long h_stride;
    float* mu; long long mu_stride;
    int rows, P;
};

// mu = softmax(h, dim=1): exp(h - max) / sum, the maximum subtracted first (expf: the accurate one, no fast-math intrinsic)
__global__ void __launch_bounds__(256) mcp_head_forward_kernel(const McpHeadFwdArgs a) {
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < a.rows; r += (long long)gridDim.x * blockDim.x) {
        const float* h = a.h + r * a.h_stride;
        float* mu = a.mu + r * a.mu_stride;
        float m = h[0];
        for (int k = 1; k < a.P; ++k) m = fmaxf(m, h[k]);
        float e[kMcpMaxPrim];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < kMcpMaxPrim; ++k) {
            if (k < a.P) { e[k] = expf(h[k] - m); s = s + e[k]; }
        }
#pragma unroll
        for (int k = 0; k < kMcpMaxPrim; ++k) {
            if (k < a.P) mu[k] = e[k] / s;
        }
    }
}

struct McpHeadBwdArgs {
    const float* dmu; long long dmu_stride;
    const float* mu; long long mu_stride;          // NULL: no softmax
    const float* aux; long long aux_stride;
    float* dz; long long dz_stride;
    int rows, P, act;
};

__device__ __forceinline__ float mcp_silu_deriv(float z) {           // d silu / d z = s (1 + z (1 - s)), s = sigmoid(z)
    const float sg = 1.f / (1.f + expf(-z));
    return sg * (1.f + z * (1.f - sg));
}

__global__ void __launch_bounds__(256) mcp_head_backward_kernel(const McpHeadBwdArgs a) {
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < a.rows; r += (long long)gridDim.x * blockDim.x) {
        const float* dmu = a.dmu + r * a.dmu_stride;
        const float* mu = a.mu ? a.mu + r * a.mu_stride : nullptr;
        const float* aux = a.aux ? a.aux + r * a.aux_stride : nullptr;
        float* dz = a.dz + r * a.dz_stride;
        float dot = 0.f;
        if (mu) {
            for (int k = 0; k < a.P; ++k) dot = dot + mu[k] * dmu[k];
        }
        for (int k = 0; k < a.P; ++k) {
            const float dh = mu ? mu[k] * (dmu[k] - dot) : dmu[k];
            float v = dh;
            if (a.act == PULSE_ACT_RELU) v = aux[k] > 0.f ? dh : 0.f;
            else if (a.act == PULSE_ACT_SILU) v = dh * mcp_silu_deriv(aux[k]);
            else if (a.act == PULSE_ACT_SILU_D) v = dh * aux[k];
            dz[k] = v;
        }
    }
}

}  // namespace pulse

using namespace pulse;

extern "C" {

int pulse_mcp_compose(const float* weights, int64_t w_stride, const float* x, int64_t x_stride, int32_t a_pitch, int32_t rows, int32_t num_prim,
                      int32_t num_actions, int32_t discrete, float* actions, int64_t actions_stride, pulse_stream_t s) {
    if (rows == 0) return PULSE_OK;
    PULSE_REQUIRE(rows > 0, "pulse_mcp_compose: rows = %d", (int)rows);
    PULSE_REQUIRE(num_prim >= 1 && num_prim <= kMcpMaxPrim, "pulse_mcp_compose: num_prim = %d (1 .. 32)", (int)num_prim);
    PULSE_REQUIRE(num_actions >= 1, "pulse_mcp_compose: num_actions = %d", (int)num_actions);
    PULSE_REQUIRE(weights && x && actions, "pulse_mcp_compose: null pointer");
    PULSE_REQUIRE(w_stride >= num_prim, "pulse_mcp_compose: w_stride %lld < num_prim %d", (long long)w_stride, (int)num_prim);
    PULSE_REQUIRE(a_pitch >= num_actions, "pulse_mcp_compose: a_pitch %d < num_actions %d", (int)a_pitch, (int)num_actions);
    PULSE_REQUIRE(x_stride >= (int64_t)num_prim * a_pitch, "pulse_mcp_compose: x_stride %lld < num_prim * a_pitch", (long long)x_stride);
    PULSE_REQUIRE(actions_stride >= num_actions, "pulse_mcp_compose: actions_stride %lld < num_actions %d", (long long)actions_stride, (int)num_actions);
    McpComposeArgs a{weights, w_stride, x, x_stride, a_pitch, actions, actions_stride, rows, num_prim, num_actions, discrete ? 1 : 0};
    long long blocks = ((long long)rows * num_actions + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(mcp_compose_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(s), a);
    return check_launch("pulse_mcp_compose");
}

int pulse_mcp_head_forward(const float* h, int64_t h_stride, int32_t rows, int32_t num_prim, float* mu, int64_t mu_stride, pulse_stream_t s) {
    if (rows == 0) return PULSE_OK;
    PULSE_REQUIRE(rows > 0, "pulse_mcp_head_forward: rows = %d", (int)rows);
    PULSE_REQUIRE(num_prim >= 1 && num_prim <= kMcpMaxPrim, "pulse_mcp_head_forward: num_prim = %d (1 .. 32)", (int)num_prim);
    PULSE_REQUIRE(h && mu, "pulse_mcp_head_forward: null pointer");
    PULSE_REQUIRE(h_stride >= num_prim && mu_stride >= num_prim, "pulse_mcp_head_forward: strides do not cover num_prim = %d columns", (int)num_prim);
    McpHeadFwdArgs a{h, h_stride, mu, mu_stride, rows, num_prim};
    long long blocks = ((long long)rows + 63) / 64;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(mcp_head_forward_kernel, dim3((unsigned)blocks), dim3(64), 0, as_stream(s), a);
    return check_launch("pulse_mcp_head_forward");
}

int pulse_mcp_head_backward(const float* dmu, int64_t dmu_stride, const float* mu, int64_t mu_stride, const float* aux, int64_t aux_stride,
                            int32_t activation, int32_t rows, int32_t num_prim, float* dz, int64_t dz_stride, pulse_stream_t s) {
    if (rows == 0) return PULSE_OK;
    PULSE_REQUIRE(rows > 0, "pulse_mcp_head_backward: rows = %d", (int)rows);
    PULSE_REQUIRE(num_prim >= 1 && num_prim <= kMcpMaxPrim, "pulse_mcp_head_backward: num_prim = %d (1 .. 32)", (int)num_prim);
    PULSE_REQUIRE(activation == PULSE_ACT_NONE || activation == PULSE_ACT_RELU || activation == PULSE_ACT_SILU || activation == PULSE_ACT_SILU_D,
                  "pulse_mcp_head_backward: activation = %d", (int)activation);
    PULSE_REQUIRE(dmu && dz, "pulse_mcp_head_backward: null pointer");
    PULSE_REQUIRE(activation == PULSE_ACT_NONE || aux, "pulse_mcp_head_backward: the activation's derivative needs aux");
    PULSE_REQUIRE(dmu_stride >= num_prim && dz_stride >= num_prim && (!mu || mu_stride >= num_prim) && (!aux || aux_stride >= num_prim),
                  "pulse_mcp_head_backward: strides do not cover num_prim = %d columns", (int)num_prim);
    McpHeadBwdArgs a{dmu, dmu_stride, mu, mu_stride, aux, aux_stride, dz, dz_stride, rows, num_prim, activation};
    long long blocks = ((long long)rows + 63) / 64;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(mcp_head_backward_kernel, dim3((unsigned)blocks), dim3(64), 0, as_stream(s), a);
    return check_launch("pulse_mcp_head_backward");
}
}
