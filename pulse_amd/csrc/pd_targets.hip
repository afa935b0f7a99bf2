// The actuation stage of the env step: the policy's action becomes the PD targets the simulator is handed.
//
// Replaces the tensor-op chain of
//   the action clamp                       phc/learning/im_amp.py:68-73 (rl_games env_step)   (torch.clamp(actions, -1, 1) before the env step; here
//                                                                                        VecTaskPythonWrapper's clip_actions)
//   Humanoid.pre_physics_step              phc/env/tasks/humanoid.py:1222-1247          (self.actions = the clamped copy; freeze_hand / freeze_toe
//                                                                                        columns of the targets set to 0)
//   Humanoid._action_to_pd_targets         phc/env/tasks/humanoid.py:1392-1394          (offset + scale * action)
//   HumanoidIm._action_to_pd_targets       phc/env/tasks/humanoid_im.py:1096-1101       (res_action: ref_dof_pos + scale * action, clamped to
//                                                                                        dof_pos -+ pi / 2 with torch.minimum / torch.maximum)
// One thread per element (grid-stride over rows * num_dof < 2^31, 32-bit index arithmetic); the three per-dof tables are 69 / 153 entries and
// are read through the caches.
// When num_dof, every row pitch and every base address is a multiple of four floats the rows move as 16-byte accesses; 69 and 153 are odd,
// so the scalar form is the common one.  Compiled with -ffp-contract=off: the product is rounded to fp32 before it is added, as the two
// eager ops do.  The clamps are written with comparisons: a NaN fails every comparison and passes through (torch.clamp), and a NaN bound
// of the residual form wins (torch.minimum / torch.maximum propagate either operand's NaN).
#include <cstdint>

#include "common.h"

namespace pulse {

struct PdTargetsArgs {
    const float* action; long long action_stride;
    const float* offset;                            // NULL: 0 (never read in the residual form)
    const float* scale;
    const unsigned char* freeze;                    // NULL: no column frozen
    const float* ref; long long ref_stride;         // NULL: the plain form
    const float* sim; long long sim_stride;
    float* clamped; long long clamped_stride;       // NULL: not kept
    float* target; long long target_stride;
    int rows, D;
    float clip;
};

constexpr float kHalfPi = 1.57079632679489661923f;  // float32(np.pi / 2): the scalar operand of dof_pos -+ np.pi / 2 in fp32

__device__ __forceinline__ float pd_clip(float x, float clip) {
    const float lo = -clip;
    float v = x < lo ? lo : x;
    v = v > clip ? clip : v;
    return v;
}

__device__ __forceinline__ float pd_target(float a, float offset, float scale, bool frozen, bool res, float ref, float sim) {
    if (frozen) return 0.f;
    const float p = scale * a;
    if (!res) return offset + p;
    const float t = ref + p;
    const float up = sim + kHalfPi, lo = sim - kHalfPi;
    const float m = (t > up || up != up) ? up : t;                  // torch.minimum(t, up)
    return (m < lo || lo != lo) ? lo : m;                           // torch.maximum(m, lo)
}

__global__ void __launch_bounds__(256) pd_targets_kernel(const PdTargetsArgs a) {
    const unsigned total = (unsigned)a.rows * (unsigned)a.D;                  // < 2^31 (checked by the host): 32-bit index arithmetic and division
    const bool res = a.ref != nullptr;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned row = i / (unsigned)a.D;
        const int c = (int)(i - row * (unsigned)a.D);
        const long long e = row;
        const float v = pd_clip(a.action[e * a.action_stride + c], a.clip);
        const float t = pd_target(v, a.offset ? a.offset[c] : 0.f, a.scale[c], a.freeze && a.freeze[c], res,
                                  res ? a.ref[e * a.ref_stride + c] : 0.f, res ? a.sim[e * a.sim_stride + c] : 0.f);
        if (a.clamped) a.clamped[e * a.clamped_stride + c] = v;
        a.target[e * a.target_stride + c] = t;
    }
}

// D, every pitch and every base address a multiple of four floats: one thread per four columns
__global__ void __launch_bounds__(256) pd_targets_vec4_kernel(const PdTargetsArgs a) {
    const int q = a.D >> 2;
    const unsigned total = (unsigned)a.rows * (unsigned)q;
    const bool res = a.ref != nullptr;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned row = i / (unsigned)q;
        const int c = (int)(i - row * (unsigned)q) << 2;
        const long long e = row;
        const float4 x = *reinterpret_cast<const float4*>(a.action + e * a.action_stride + c);
        const float4 sc = *reinterpret_cast<const float4*>(a.scale + c);
        float4 of = make_float4(0.f, 0.f, 0.f, 0.f), rf = of, sm = of;
        if (a.offset) of = *reinterpret_cast<const float4*>(a.offset + c);
        if (res) {
            rf = *reinterpret_cast<const float4*>(a.ref + e * a.ref_stride + c);
            sm = *reinterpret_cast<const float4*>(a.sim + e * a.sim_stride + c);
        }
        unsigned fz = 0;
        if (a.freeze) fz = *reinterpret_cast<const unsigned*>(a.freeze + c);
        float4 v, t;
        v.x = pd_clip(x.x, a.clip); v.y = pd_clip(x.y, a.clip); v.z = pd_clip(x.z, a.clip); v.w = pd_clip(x.w, a.clip);
        t.x = pd_target(v.x, of.x, sc.x, (fz & 0x000000ffu) != 0, res, rf.x, sm.x);
        t.y = pd_target(v.y, of.y, sc.y, (fz & 0x0000ff00u) != 0, res, rf.y, sm.y);
        t.z = pd_target(v.z, of.z, sc.z, (fz & 0x00ff0000u) != 0, res, rf.z, sm.z);
        t.w = pd_target(v.w, of.w, sc.w, (fz & 0xff000000u) != 0, res, rf.w, sm.w);
        if (a.clamped) *reinterpret_cast<float4*>(a.clamped + e * a.clamped_stride + c) = v;
        *reinterpret_cast<float4*>(a.target + e * a.target_stride + c) = t;
    }
}

static bool pd_vec4_ok(const PdTargetsArgs& a) {
    auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    auto rows = [&](const void* p, long long stride) { return !p || (al(p) && (stride & 3) == 0); };
    return (a.D & 3) == 0 && rows(a.action, a.action_stride) && rows(a.ref, a.ref_stride) && rows(a.sim, a.sim_stride) &&
           rows(a.clamped, a.clamped_stride) && rows(a.target, a.target_stride) && al(a.scale) && (!a.offset || al(a.offset)) &&
           (!a.freeze || (reinterpret_cast<uintptr_t>(a.freeze) & 3u) == 0);
}

}  // namespace pulse

using namespace pulse;

extern "C" {

int pulse_pd_targets(const float* action, int64_t action_stride, int32_t rows, int32_t num_dof, float clip, const float* offset, const float* scale,
                     const uint8_t* freeze, const float* ref_dof_pos, int64_t ref_stride, const float* sim_dof_pos, int64_t sim_stride,
                     float* clamped, int64_t clamped_stride, float* target, int64_t target_stride, pulse_stream_t s) {
    if (rows == 0) return PULSE_OK;
    PULSE_REQUIRE(rows > 0 && num_dof >= 1, "pulse_pd_targets: rows = %d, num_dof = %d", (int)rows, (int)num_dof);
    PULSE_REQUIRE((long long)rows * num_dof < (1ll << 31), "pulse_pd_targets: rows * num_dof = %lld (the kernel indexes elements with 32 bits)",
                  (long long)rows * num_dof);
    PULSE_REQUIRE(action && scale && target, "pulse_pd_targets: null pointer (action / scale / target)");
    PULSE_REQUIRE(clip >= 0.f, "pulse_pd_targets: clip = %g (a bound >= 0, inf for none)", (double)clip);
    PULSE_REQUIRE((ref_dof_pos != nullptr) == (sim_dof_pos != nullptr), "pulse_pd_targets: the residual form takes ref_dof_pos AND sim_dof_pos");
    PULSE_REQUIRE(action_stride >= num_dof && target_stride >= num_dof && (!clamped || clamped_stride >= num_dof) &&
                  (!ref_dof_pos || (ref_stride >= num_dof && sim_stride >= num_dof)),
                  "pulse_pd_targets: a row stride does not cover num_dof = %d columns", (int)num_dof);
    PdTargetsArgs a{action, action_stride, offset, scale, freeze, ref_dof_pos, ref_stride, sim_dof_pos, sim_stride,
                    clamped, clamped_stride, target, target_stride, rows, num_dof, clip};
    const bool vec = pd_vec4_ok(a);
    long long blocks = ((long long)rows * (vec ? num_dof / 4 : num_dof) + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (vec) hipLaunchKernelGGL(pd_targets_vec4_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(s), a);
    else hipLaunchKernelGGL(pd_targets_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(s), a);
    return check_launch("pulse_pd_targets");
}
}
