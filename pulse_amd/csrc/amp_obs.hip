// AMP (adversarial motion prior) per-frame observation for gfx950.
//
// Replaces build_amp_observations_smpl (phc/env/tasks/humanoid_amp.py:925-969) and dof_to_obs_smpl
// (phc/env/tasks/humanoid.py:1436-1446): per env
//   [root_h (1)?, 6-D heading-local root rot, local root lin vel (3), local root ang vel (3),
//    6-D rotation of every (selected) dof joint from its exp-map (6 Jd), dof velocities (3 Jd),
//    heading-local key-body positions (3 Kb)]
// = 232 floats for the 23 SMPL joints / 4 key bodies (196 for the 19-joint subset), and its configured variants:
//   * version 2 (build_amp_observations_smpl_v2, :973-1017): + heading-local key-body velocities (3 Kb) behind the positions;
//   * has_shape_obs_disc / has_limb_weight_obs_disc (:963-966): + the env's (the motion's, for reference frames) shape / limb rows, copied;
//   * has_upright_start False (:929-930): the root rotation goes through remove_base_rot (humanoid.py:1617-1620) before anything reads it.
//
// Same mapping as the fused env step: a 32-lane half-wave per env, lane j <-> joint j / key body j, inputs
// read straight from the 13-float rigid-body records and the (N, 69) dof tensors, the feature row assembled
// in LDS and written with coalesced stores into the caller's pitch (e.g. slot 0 of the (N, 10, W) history).
// HBM/launch bound: 52 B root record + 2 x 276 B dofs + 48 B key bodies read, 4 W bytes written per env.
// Compiled with -ffp-contract=off (reference operation order).
#include "env_select.h"
#include "motion_math.h"

namespace pulse {

constexpr int kAmpLanes = kHalfWave, kAmpThreads = 128, kAmpEnvs = LaneGroup<kAmpLanes, kAmpThreads>::slots;
constexpr int kAmpMaxW = 320;

constexpr int kAmpMaxHist = 9;      // history frames behind the current one (numAMPObsSteps - 1)

// column offsets of one frame: [h?, rot6, vel3, angvel3, 6 Jd, 3 Jd, 3 Kb, (v2: 3 Kb), num_shape, num_limb]
struct AmpLayout { int h0, off_vel, off_ang, off_dof, off_dvel, off_key, off_kvel, off_shape, off_limb, W; };

__host__ __device__ inline AmpLayout amp_layout(int Jd, int Kb, int root_height_obs, int version, int num_shape, int num_limb) {
    AmpLayout L;
    L.h0 = root_height_obs ? 1 : 0;
    L.off_vel = L.h0 + 6; L.off_ang = L.off_vel + 3; L.off_dof = L.off_ang + 3; L.off_dvel = L.off_dof + 6 * Jd; L.off_key = L.off_dvel + 3 * Jd;
    L.off_kvel = L.off_key + 3 * Kb;
    L.off_shape = L.off_kvel + (version == 2 ? 3 * Kb : 0);
    L.off_limb = L.off_shape + num_shape;
    L.W = L.off_limb + num_limb;
    return L;
}

// the shape / limb rows behind everything else (copied, never computed)
__device__ __forceinline__ void amp_copy_rows(float* o, const AmpLayout& L, int lane, const float* shape, int num_shape, const float* limb, int num_limb) {
    for (int c = lane; c < num_shape; c += kAmpLanes) o[L.off_shape + c] = shape[c];
    for (int c = lane; c < num_limb; c += kAmpLanes) o[L.off_limb + c] = limb[c];
}

// HIST: ``out`` is slot 0 of the env's (hist_steps, W) history window (HumanoidAMP._amp_obs_buf, humanoid_amp.py:296-314).  The launch
// then does the whole per-step update of HumanoidAMP.post_physics_step (:194-210) for the env: _update_hist_amp_obs (frames 0 .. S-2 move
// to 1 .. S-1, :622-631), the current frame into slot 0, and -- window_out -- the finished window copied to the caller's row (the
// experience-buffer slot of this rollout step: amp_agent.py:377).  Four device copies of the (N, S W) window become none.
// vec4 (uniform over the launch, set by the launcher): W, both pitches and both bases are multiples of 16 bytes, so the three copies of the
// history run as float4 loops; otherwise (e.g. W = 207, the shape-aware 19-joint frame) the same copies run float by float.
// PLAIN: the upright, version-1 frame without rows on aligned windows -- the shipped SMPL configuration -- with the variant switches folded at
// compile time (measured: as runtime flags they cost the fused cfg5 launch 0.6 us of 46, profiles/amp_obs_variants_ab.txt).
template <bool HIST, bool PLAIN>
__global__ void __launch_bounds__(kAmpThreads) amp_obs_kernel(const pulse_amp_obs_args a, const int vec4_arg) {
    const int vec4 = PLAIN ? 1 : vec4_arg, version = PLAIN ? 1 : a.version, upright_start = PLAIN ? 1 : a.upright_start;
    const int num_shape = PLAIN ? 0 : a.num_shape, num_limb = PLAIN ? 0 : a.num_limb;
    __shared__ __align__(16) float s_out[kAmpEnvs][kAmpMaxW];
    __shared__ __align__(16) float s_hist[HIST ? kAmpEnvs : 1][HIST ? kAmpMaxHist * kAmpMaxW : 1];
    const auto [slot, lane, idx] = lane_group<kAmpLanes, kAmpThreads>();
    int64_t e = 0;
    const bool valid = select_env(a, (int)idx, e);                           // (carried past the barrier: nobody returns early)
    const int Jd = a.num_joints, Kb = a.num_key_bodies;
    const AmpLayout L = amp_layout(Jd, Kb, a.root_height_obs, version, num_shape, num_limb);   // counts are 0 without a pointer (launcher)
    const int h0 = L.h0, off_vel = L.off_vel, off_ang = L.off_ang, off_dof = L.off_dof, off_dvel = L.off_dvel, off_key = L.off_key, W = L.W;
    float* o = s_out[slot];
    if constexpr (HIST) {
        if (valid) {                                                     // the frames that move down one slot (read before anything is written)
            const float* h = a.out + e * a.out_stride;
            const int nh = (a.hist_steps - 1) * W;
            if (vec4) {
                const int n4 = nh / 4;
                for (int c = lane; c < n4; c += kAmpLanes) reinterpret_cast<float4*>(s_hist[slot])[c] = reinterpret_cast<const float4*>(h)[c];
            } else {
                for (int c = lane; c < nh; c += kAmpLanes) s_hist[slot][c] = h[c];
            }
        }
    }
    if (valid) {
        const float* rb = a.rb + e * a.rb_env_stride;
        const V3 root_p{rb[0], rb[1], rb[2]};
        const Q4 root_q = remove_base_rot(Q4{rb[3], rb[4], rb[5], rb[6]}, upright_start);
        const Q4 hinv = heading_quat(root_q, true);
        if (lane == 0) {
            if (a.root_height_obs) o[0] = root_p.z;
            float tn[6];
            q_to_tan_norm(a.local_root_obs ? qmul(hinv, root_q) : root_q, tn);
#pragma unroll
            for (int k = 0; k < 6; ++k) o[h0 + k] = tn[k];
            const V3 lv = qrot(hinv, V3{rb[7], rb[8], rb[9]});
            const V3 lw = qrot(hinv, V3{rb[10], rb[11], rb[12]});
            o[off_vel] = lv.x; o[off_vel + 1] = lv.y; o[off_vel + 2] = lv.z;
            o[off_ang] = lw.x; o[off_ang + 1] = lw.y; o[off_ang + 2] = lw.z;
        }
        if (lane < Jd) {
            const int j = a.joint_ids ? a.joint_ids[lane] : lane;
            const bool zeroed = a.zero_joint_mask & (1u << j);     // the "ZL hack" (humanoid_amp.py:636-639): toes / hands read as 0
            const float* dp = a.dof_pos + e * a.num_dof + 3 * j;
            const float* dv = a.dof_vel + e * a.num_dof + 3 * j;
            const V3 em = zeroed ? V3{0.f, 0.f, 0.f} : V3{dp[0], dp[1], dp[2]};
            float tn[6];
            q_to_tan_norm(exp_map_to_q(em), tn);
#pragma unroll
            for (int k = 0; k < 6; ++k) o[off_dof + 6 * lane + k] = tn[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) o[off_dvel + 3 * lane + k] = zeroed ? 0.f : dv[k];
        }
        if (lane < Kb) {
            const float* kb = rb + 13 * a.key_body_ids[lane];
            const V3 lp = qrot(hinv, V3{kb[0] - root_p.x, kb[1] - root_p.y, kb[2] - root_p.z});
            o[off_key + 3 * lane] = lp.x; o[off_key + 3 * lane + 1] = lp.y; o[off_key + 3 * lane + 2] = lp.z;
            if (version == 2) {                                        // key-body velocities, floats 7..9 of the body's record (:999)
                const V3 lkv = qrot(hinv, V3{kb[7], kb[8], kb[9]});
                o[L.off_kvel + 3 * lane] = lkv.x; o[L.off_kvel + 3 * lane + 1] = lkv.y; o[L.off_kvel + 3 * lane + 2] = lkv.z;
            }
        }
        amp_copy_rows(o, L, lane, a.shape_params + e * a.shape_stride, num_shape, a.limb_weights + e * a.limb_stride, num_limb);
    }
    __syncthreads();
    if (valid) {
        float* g = a.out + e * a.out_stride;
        for (int c = lane; c < W; c += kAmpLanes) g[c] = o[c];
        if constexpr (HIST) {
            const int nh = (a.hist_steps - 1) * W;
            if (vec4) {
                const int n4 = nh / 4, w4 = W / 4;
                float4* gh = reinterpret_cast<float4*>(g + W);
                const float4* sh = reinterpret_cast<const float4*>(s_hist[slot]);
                for (int c = lane; c < n4; c += kAmpLanes) gh[c] = sh[c];
                if (a.window_out) {
                    float* wo = a.window_out + e * a.window_stride;
                    for (int c = lane; c < w4; c += kAmpLanes) reinterpret_cast<float4*>(wo)[c] = reinterpret_cast<const float4*>(o)[c];
                    float4* wh = reinterpret_cast<float4*>(wo + W);
                    for (int c = lane; c < n4; c += kAmpLanes) wh[c] = sh[c];
                }
            } else {
                const float* sh = s_hist[slot];
                for (int c = lane; c < nh; c += kAmpLanes) g[W + c] = sh[c];
                if (a.window_out) {
                    float* wo = a.window_out + e * a.window_stride;
                    for (int c = lane; c < W; c += kAmpLanes) wo[c] = o[c];
                    for (int c = lane; c < nh; c += kAmpLanes) wo[W + c] = sh[c];
                }
            }
        }
    }
}

// _init_amp_obs_ref (humanoid_amp.py:531-563) for the masked envs in ONE launch: history slot k + 1 of env e := the AMP frame of the
// env's motion at start_time[e] - dt (k + 1) -- MotionLib.get_motion_state (motion_lib_base.py:434-517) and build_amp_observations_smpl
// fused, a half-wave per (env, k); envs outside the mask cost an index read.  (Was: a motion query and an AMP-frame pass over ALL
// N x (S - 1) rows plus a where / copy of the window, 195 us per rollout step at 8192 envs.)
__global__ void __launch_bounds__(kAmpThreads) amp_hist_init_kernel(const pulse_amp_hist_args a) {
    __shared__ float s_out[kAmpEnvs][kAmpMaxW];
    const auto [slot, lane, idx] = lane_group<kAmpLanes, kAmpThreads>();
    const int Hs = a.hist_steps - 1;
    bool valid = idx < (long long)a.num_envs * Hs;
    const long long e = valid ? idx / Hs : 0;
    const int k = valid ? (int)(idx - e * Hs) : 0;
    valid = valid && env_enabled(a, e);
    const int Jd = a.num_joints, Kb = a.num_key_bodies;
    const AmpLayout L = amp_layout(Jd, Kb, a.root_height_obs, a.version, a.num_shape, a.num_limb);   // counts are 0 without a pointer (launcher)
    const int h0 = L.h0, off_vel = L.off_vel, off_ang = L.off_ang, off_dof = L.off_dof, off_dvel = L.off_dvel, off_key = L.off_key, W = L.W;
    float* o = s_out[slot];
    if (valid) {
        const pulse_motion_tables& T = a.tab;
        // times = start_times[:, None] + (-dt * (arange(S - 1) + 1))   (fp32, the reference's op order)
        const float t = a.start_times[e] + (float)(k + 1) * (-a.dt);
        const FramePair fp = frame_pair(T, a.motion_ids[e], t);
        BodyState root = blend_body(T, fp.r0, fp.r1, fp.blend, 0, nullptr);
        root.q = remove_base_rot(root.q, a.upright_start);
        const Q4 hinv = heading_quat(root.q, true);
        if (lane == 0) {
            if (a.root_height_obs) o[0] = root.p.z;
            float tn[6];
            q_to_tan_norm(a.local_root_obs ? qmul(hinv, root.q) : root.q, tn);
#pragma unroll
            for (int c = 0; c < 6; ++c) o[h0 + c] = tn[c];
            const V3 lv = qrot(hinv, root.v), lw = qrot(hinv, root.w);
            o[off_vel] = lv.x; o[off_vel + 1] = lv.y; o[off_vel + 2] = lv.z;
            o[off_ang] = lw.x; o[off_ang + 1] = lw.y; o[off_ang + 2] = lw.z;
        }
        if (lane < Jd) {
            const int j = a.joint_ids ? a.joint_ids[lane] : lane;
            V3 dp, dv;
            blend_dof(T, fp.r0, fp.r1, fp.blend, j, &dp, &dv);
            float tn[6];
            q_to_tan_norm(exp_map_to_q(dp), tn);
#pragma unroll
            for (int c = 0; c < 6; ++c) o[off_dof + 6 * lane + c] = tn[c];
            o[off_dvel + 3 * lane] = dv.x; o[off_dvel + 3 * lane + 1] = dv.y; o[off_dvel + 3 * lane + 2] = dv.z;
        }
        if (lane < Kb) {
            const int b = a.key_body_ids[lane];
            const V3 kp = lerp3(fp.r0 + T.off_gts + 3 * b, fp.r1 + T.off_gts + 3 * b, fp.blend);
            const V3 lp = qrot(hinv, V3{kp.x - root.p.x, kp.y - root.p.y, kp.z - root.p.z});
            o[off_key + 3 * lane] = lp.x; o[off_key + 3 * lane + 1] = lp.y; o[off_key + 3 * lane + 2] = lp.z;
            if (a.version == 2) {                                      // body_vel[:, key] (:553), blended as blend_body does
                const V3 kv = lerp3(fp.r0 + T.off_gvs + 3 * b, fp.r1 + T.off_gvs + 3 * b, fp.blend);
                const V3 lkv = qrot(hinv, kv);
                o[L.off_kvel + 3 * lane] = lkv.x; o[L.off_kvel + 3 * lane + 1] = lkv.y; o[L.off_kvel + 3 * lane + 2] = lkv.z;
            }
        }
        const long long m = a.motion_ids[e];                           // the motion's rows (motion_bodies / motion_limb_weights, :548-555)
        amp_copy_rows(o, L, lane, a.shape_params + m * a.shape_stride, a.num_shape, a.limb_weights + m * a.limb_stride, a.num_limb);
    }
    __syncthreads();
    if (valid) {
        float* g = a.hist + e * a.env_stride + (long long)(k + 1) * a.step_stride;
        for (int c = lane; c < W; c += kAmpLanes) g[c] = o[c];
    }
}

// the checks both entries share: version, row pointers / counts / pitches
template <class Args>
int amp_check_variant(const Args& a, const char* name) {
    PULSE_REQUIRE(a.version == 1 || a.version == 2, "%s: version must be 1 or 2", name);
    PULSE_REQUIRE(a.num_shape >= 0 && a.num_limb >= 0 && (a.shape_params || a.num_shape == 0) && (a.limb_weights || a.num_limb == 0) &&
                  (!a.shape_params || a.shape_stride >= a.num_shape) && (!a.limb_weights || a.limb_stride >= a.num_limb),
                  "%s: shape / limb rows need a pointer, a count >= 0 and a pitch >= the count", name);
    return PULSE_OK;
}

}  // namespace pulse

using namespace pulse;

extern "C" {

int pulse_sizeof_amp_obs_args(void) { return (int)sizeof(pulse_amp_obs_args); }

int pulse_amp_obs_width(int num_joints, int num_key_bodies, int root_height_obs) {
    return (root_height_obs ? 1 : 0) + 12 + 9 * num_joints + 3 * num_key_bodies;
}

int pulse_amp_obs_width_v(int num_joints, int num_key_bodies, int root_height_obs, int version, int num_shape, int num_limb) {
    return amp_layout(num_joints, num_key_bodies, root_height_obs, version, num_shape, num_limb).W;
}

int pulse_amp_obs(const pulse_amp_obs_args* args, pulse_stream_t s) {
    PULSE_REQUIRE(args != nullptr, "pulse_amp_obs: null args");
    const pulse_amp_obs_args& a = *args;
    const int count = env_count(a);
    PULSE_REQUIRE(count >= 0, "pulse_amp_obs: negative count");
    if (count == 0) return PULSE_OK;
    PULSE_REQUIRE(a.rb && a.dof_pos && a.dof_vel && a.out && a.key_body_ids, "pulse_amp_obs: null pointer");
    PULSE_REQUIRE(a.num_joints >= 1 && a.num_joints <= kAmpLanes && a.num_key_bodies >= 0 && a.num_key_bodies <= kAmpLanes,
                  "pulse_amp_obs: joints / key bodies must fit 32 lanes");
    PULSE_REQUIRE(a.num_dof >= 3 * a.num_joints || a.joint_ids, "pulse_amp_obs: num_dof too small");
    if (const int rc = amp_check_variant(a, "pulse_amp_obs")) return rc;
    const int w = pulse_amp_obs_width_v(a.num_joints, a.num_key_bodies, a.root_height_obs, a.version, a.num_shape, a.num_limb);
    PULSE_REQUIRE(w <= kAmpMaxW && a.out_stride >= w, "pulse_amp_obs: width %d exceeds %d or the output pitch", w, kAmpMaxW);
    const bool plain = a.upright_start && a.version == 1 && a.num_shape == 0 && a.num_limb == 0;
    unsigned blocks;
    if (const int rc = lane_group_blocks("pulse_amp_obs", count, kAmpEnvs, blocks)) return rc;
    const dim3 grid(blocks), block(kAmpThreads);
    if (a.hist_steps > 1) {
        PULSE_REQUIRE(a.hist_steps - 1 <= kAmpMaxHist && a.out_stride >= (int64_t)a.hist_steps * w,
                      "pulse_amp_obs: history mode needs hist_steps <= %d and a window pitch of hist_steps * W floats", kAmpMaxHist + 1);
        PULSE_REQUIRE(!a.window_out || a.window_stride >= (int64_t)a.hist_steps * w, "pulse_amp_obs: window_out rows must hold hist_steps * W floats");
        // float4 copies when every row of both windows starts on 16 bytes and W is a multiple of 4 floats; float by float otherwise
        const int vec4 = (w % 4) == 0 && (a.out_stride % 4) == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0 &&
                         (!a.window_out || ((a.window_stride % 4) == 0 && (reinterpret_cast<uintptr_t>(a.window_out) & 15) == 0));
        if (plain && vec4) hipLaunchKernelGGL((amp_obs_kernel<true, true>), grid, block, 0, as_stream(s), a, 1);
        else hipLaunchKernelGGL((amp_obs_kernel<true, false>), grid, block, 0, as_stream(s), a, vec4);
    } else {
        PULSE_REQUIRE(a.window_out == nullptr, "pulse_amp_obs: window_out goes with hist_steps > 1");
        if (plain) hipLaunchKernelGGL((amp_obs_kernel<false, true>), grid, block, 0, as_stream(s), a, 0);
        else hipLaunchKernelGGL((amp_obs_kernel<false, false>), grid, block, 0, as_stream(s), a, 0);
    }
    return check_launch("pulse_amp_obs");
}

int pulse_sizeof_amp_hist_args(void) { return (int)sizeof(pulse_amp_hist_args); }

int pulse_amp_hist_init(const pulse_amp_hist_args* args, pulse_stream_t s) {
    PULSE_REQUIRE(args != nullptr, "pulse_amp_hist_init: null args");
    const pulse_amp_hist_args& a = *args;
    PULSE_REQUIRE(a.num_envs >= 0 && a.hist_steps >= 1, "pulse_amp_hist_init: bad sizes");
    if (a.num_envs == 0 || a.hist_steps == 1) return PULSE_OK;
    const pulse_motion_tables& T = a.tab;
    if (const int rc = check_motion_tables("pulse_amp_hist_init", T, kAmpLanes)) return rc;
    PULSE_REQUIRE(a.motion_ids && a.start_times && a.hist && a.key_body_ids, "pulse_amp_hist_init: null pointer");
    PULSE_REQUIRE(a.num_joints >= 1 && a.num_joints <= kAmpLanes && (a.joint_ids || a.num_joints <= T.num_bodies - 1) &&
                  a.num_key_bodies >= 0 && a.num_key_bodies <= kAmpLanes, "pulse_amp_hist_init: joints / key bodies must fit 32 lanes and the skeleton");
    if (const int rc = amp_check_variant(a, "pulse_amp_hist_init")) return rc;
    const int w = pulse_amp_obs_width_v(a.num_joints, a.num_key_bodies, a.root_height_obs, a.version, a.num_shape, a.num_limb);
    PULSE_REQUIRE(w <= kAmpMaxW && a.step_stride >= w && a.env_stride >= (int64_t)a.hist_steps * a.step_stride, "pulse_amp_hist_init: bad pitches");
    unsigned blocks;
    if (const int rc = lane_group_blocks("pulse_amp_hist_init", (long long)a.num_envs * (a.hist_steps - 1), kAmpEnvs, blocks)) return rc;
    hipLaunchKernelGGL(amp_hist_init_kernel, dim3(blocks), dim3(kAmpThreads), 0, as_stream(s), a);
    return check_launch("pulse_amp_hist_init");
}
}
