// What the env-side kernels (task_step, traj_step, crowd_obs, amp_obs, eval_metrics) open and close with: which env a launch slot stands for,
// and compute_humanoid_reset's fall test.  Templated on the argument struct of include/pulse_hip.h: every struct spells these fields alike.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pulse {

// slots of a launch: the id list's length, or every env (kernels and C entry points)
template <typename Args>
__host__ __device__ __forceinline__ int env_count(const Args& a) { return a.env_ids ? a.num_ids : a.num_envs; }

// env e exists and its mask byte, if there is a mask, is set (the whole selection of a struct without an id list)
template <typename Args>
__device__ __forceinline__ bool env_enabled(const Args& a, int64_t e) {
    if (e < 0 || e >= a.num_envs) return false;
    return !(a.env_mask && a.env_mask[e] == 0);
}

// slot idx -> env e.  False (e then means nothing): idx past the count, an id outside [0, num_envs), or a masked env.  Kernels without a
// barrier return on false; the ones that go on to a barrier keep the result as their ``valid`` flag.
template <typename Args>
__device__ __forceinline__ bool select_env(const Args& a, int idx, int64_t& e) {
    if (idx >= env_count(a)) return false;
    e = a.env_ids ? a.env_ids[idx] : (int64_t)idx;
    return env_enabled(a, e);
}

// compute_humanoid_reset's fall test (phc/env/tasks/humanoid.py:1572-1608): over the bodies outside contact_body_ids, some |force component|
// above 0.1 AND some body below its termination height.  rb: the env's 13-float records, cf: its (num_bodies, 3) contact forces.
// per_body(b, |f|) sees every body the test looks at (the strike task's extra force test rides on it).
template <typename Args, typename PerBody>
__device__ __forceinline__ bool has_fallen(const Args& a, const float* rb, const float* cf, PerBody per_body) {
    bool fall_contact = false, fall_height = false;
    for (int b = 0; b < a.num_bodies; ++b) {
        bool is_contact_body = false;
        for (int k = 0; k < a.num_contact_ids; ++k) is_contact_body |= a.contact_body_ids[k] == b;
        if (is_contact_body) continue;                           // masked_contact_buf[:, contact_body_ids, :] = 0
        const float ax = fabsf(cf[3 * b]), ay = fabsf(cf[3 * b + 1]), az = fabsf(cf[3 * b + 2]);
        fall_contact |= (ax > 0.1f) || (ay > 0.1f) || (az > 0.1f);
        fall_height |= rb[13 * b + 2] < a.termination_heights[b];
        per_body(b, ax, ay, az);
    }
    return fall_contact && fall_height;
}

}  // namespace pulse
