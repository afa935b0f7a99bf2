// Reference-state reset of the downstream tasks for gfx950: HumanoidAMP._reset_ref_state_init / _sample_ref_state
// (phc/env/tasks/humanoid_amp.py:447-488) with the four task overrides of _sample_ref_state
//   HumanoidTraj                  none                                  humanoid_amp.py:447-466
//   HumanoidReach / Strike        root xy = 0                           humanoid_reach.py:46-49, humanoid_strike.py:147-150
//   HumanoidSpeed                 heading removed about the root        humanoid_speed.py:251-270
//   HumanoidPedestrianTerrain     moved to new_root_xy, lifted by the mean centre height      humanoid_pedestrian_terrain.py:488-589
// in ONE launch: blend of the clip at (motion id, time) with the device functions of motion_math.h (same expressions, same order as
// pulse_motion_state), the task's root transform, the 13-float records of all bodies, dof_pos / dof_vel, start time, motion id, and up to
// three cleared per-env words.
//
// What the records hold: the root record is exactly what the reference hands to the simulator as the root state; every other body is
// carried rigidly by the same root transform.  The reference's transient _rigid_body_* cache differs in three places (speed: body_ang_vel
// not turned; reach / strike: bodies not translated; terrain: bodies never lifted) until Isaac's next refresh rebuilds it from the root and
// dof state -- include/pulse_hip.h, DESIGN.md section 1.
//
// Mapping: a 32-lane half-wave per env, lane = body (<= 32 bodies), eight envs per 256-thread workgroup as in motion_state.hip.  The root
// state every lane needs goes through LDS (no cross-lane instruction: the two halves of a wave diverge on their mask flags); the finished
// rows are put together in LDS (lane strides 13 and 3 floats: odd, conflict-free) and stored with adjacent lanes on adjacent addresses.
// An env outside the mask reads its flag and writes nothing.  HBM bound: 2 x 1908 B read, 1.8 KB written per masked env.
// Compiled with -ffp-contract=off (reference operation order).
#include "motion_math.h"
#include "terrain_math.h"

namespace pulse {

constexpr int kTrLanes = kHalfWave, kTrThreads = LaneGroup<kTrLanes>::threads, kTrEnvs = LaneGroup<kTrLanes>::slots;      // lanes per env = the most bodies
constexpr int kTrRec = 13 * kTrLanes;
constexpr int kTrDof = 3 * (kTrLanes - 1);

__global__ void __launch_bounds__(kTrThreads) task_reset_kernel(const pulse_task_reset_args a) {
    __shared__ float s_rec[kTrEnvs][kTrRec];
    __shared__ float s_dp[kTrEnvs][kTrDof];
    __shared__ float s_dv[kTrEnvs][kTrDof];
    __shared__ float s_root[kTrEnvs][8];              // blended root: position, rotation
    __shared__ float s_cpt[kTrEnvs][kTrLanes];        // centre-grid heights
    const auto [slot, lane, e] = lane_group<kTrLanes>();
    const pulse_motion_tables& T = a.tab;
    const int J = T.num_bodies;
    long long m = 0;
    bool active = e < a.num_envs && a.env_mask[e] != 0;
    if (active) {
        m = a.motion_ids[e];
        active = m >= 0 && m < T.num_motions;
    }
    float t = 0.0f;
    BodyState s{};
    if (active) {
        t = a.times[e];
        const FramePair fp = frame_pair(T, m, t);
        if (lane < J) {
            s = blend_body(T, fp.r0, fp.r1, fp.blend, lane, nullptr);
            if (lane == 0) {
                float* r = s_root[slot];
                r[0] = s.p.x; r[1] = s.p.y; r[2] = s.p.z; r[3] = s.q.x; r[4] = s.q.y; r[5] = s.q.z; r[6] = s.q.w;
            }
        }
        if (lane < J - 1) {
            V3 dp, dv;
            blend_dof(T, fp.r0, fp.r1, fp.blend, lane, &dp, &dv);
            float* o = s_dp[slot] + 3 * lane;
            o[0] = dp.x; o[1] = dp.y; o[2] = dp.z;
            o = s_dv[slot] + 3 * lane;
            o[0] = dv.x; o[1] = dv.y; o[2] = dv.z;
        }
    }
    __syncthreads();
    const float* r = s_root[slot];
    const V3 rp{r[0], r[1], r[2]};
    const Q4 rq{r[3], r[4], r[5], r[6]};
    float nx = 0.0f, ny = 0.0f;
    if (active && a.transform == PULSE_TASK_RESET_TERRAIN) {
        nx = a.new_root_xy[2 * e];
        ny = a.new_root_xy[2 * e + 1];
        if (a.heightsamples && lane < a.num_center_points) {
            // get_center_heights (:690-716) of the MOVED root: the grid turned by the root's yaw only
            const HeightField hf = height_field_of(a);
            const V3 w = q_apply(yaw_quat(remove_base_rot(rq, a.upright_start)), V3{a.center_points[2 * lane], a.center_points[2 * lane + 1], 0.0f});
            s_cpt[slot][lane] = sample_height(hf, w.x + nx, w.y + ny);
        }
    }
    __syncthreads();
    if (active && lane < J) {
        if (a.transform == PULSE_TASK_RESET_ZERO_XY) {
            // root_pos[..., :2] = 0; the other bodies go with the root
            s.p.x = lane == 0 ? 0.0f : s.p.x - rp.x;
            s.p.y = lane == 0 ? 0.0f : s.p.y - rp.y;
        } else if (a.transform == PULSE_TASK_RESET_REMOVE_HEADING) {
            const Q4 hinv = heading_quat(remove_base_rot(rq, a.upright_start), true);
            const V3 d = q_apply(hinv, V3{s.p.x - rp.x, s.p.y - rp.y, s.p.z - rp.z});               // quat_apply(h, rb_pos - root_pos) + root_pos
            s.p = V3{d.x + rp.x, d.y + rp.y, d.z + rp.z};
            s.q = qmul(hinv, s.q);
            s.v = q_apply(hinv, s.v);
            s.w = q_apply(hinv, s.w);
        } else if (a.transform == PULSE_TASK_RESET_TERRAIN) {
            float center = 0.0f;
            if (a.heightsamples) {
                float sum = 0.0f;
                for (int c = 0; c < a.num_center_points; ++c) sum += s_cpt[slot][c];
                center = sum / (float)a.num_center_points;
            }
            // diff_xy = new_root_xy - root_pos[:, 0:2]; root_pos[:, 0:2] = new_root_xy; root_pos[:, 2] += center_height
            const float dx = nx - rp.x, dy = ny - rp.y;
            s.p.x = lane == 0 ? nx : s.p.x + dx;
            s.p.y = lane == 0 ? ny : s.p.y + dy;
            s.p.z = s.p.z + center;
        }
        store_record(s_rec[slot] + 13 * lane, s);
    }
    __syncthreads();
    if (!active) return;
    float* rb = a.rb + e * a.rb_env_stride;
    for (int i = lane; i < 13 * J; i += kTrLanes) rb[i] = s_rec[slot][i];
    const int nd = 3 * (J - 1);
    float* dp = a.dof_pos + e * nd;
    float* dv = a.dof_vel + e * nd;
    for (int i = lane; i < nd; i += kTrLanes) { dp[i] = s_dp[slot][i]; dv[i] = s_dv[slot][i]; }
    if (lane == 0) {
        a.start_times[e] = t;
        a.sampled_ids[e] = m;
        if (a.clear0) a.clear0[e] = 0;
        if (a.clear1) a.clear1[e] = 0;
        if (a.clear2) a.clear2[e] = 0;
    }
}

}  // namespace pulse

extern "C" int pulse_sizeof_task_reset_args(void) { return (int)sizeof(pulse_task_reset_args); }

extern "C" int pulse_task_ref_state_init(const pulse_task_reset_args* args, pulse_stream_t s) {
    using namespace pulse;
    PULSE_REQUIRE(args != nullptr, "pulse_task_ref_state_init: null args");
    const pulse_task_reset_args& a = *args;
    const pulse_motion_tables& T = a.tab;
    PULSE_REQUIRE(a.num_envs >= 0, "pulse_task_ref_state_init: negative num_envs");
    PULSE_REQUIRE(T.num_bodies >= 2 && T.num_bodies <= kTrLanes, "pulse_task_ref_state_init: num_bodies %d not in [2,32] (a 32-lane half-wave per env, lane = body)",
                  T.num_bodies);
    if (a.num_envs == 0) return PULSE_OK;
    if (const int rc = check_motion_tables("pulse_task_ref_state_init", T, kTrLanes)) return rc;
    PULSE_REQUIRE(a.transform >= PULSE_TASK_RESET_NONE && a.transform <= PULSE_TASK_RESET_TERRAIN, "pulse_task_ref_state_init: unknown transform %d", a.transform);
    PULSE_REQUIRE(a.env_mask && a.motion_ids && a.times, "pulse_task_ref_state_init: null env_mask / motion_ids / times");
    PULSE_REQUIRE(a.rb && a.rb_env_stride >= 13LL * T.num_bodies && a.dof_pos && a.dof_vel && a.start_times && a.sampled_ids,
                  "pulse_task_ref_state_init: null output or rb_env_stride too small");
    if (a.transform == PULSE_TASK_RESET_TERRAIN) {
        PULSE_REQUIRE(a.new_root_xy, "pulse_task_ref_state_init: TERRAIN needs new_root_xy");
        PULSE_REQUIRE(!a.heightsamples || (a.map_rows >= 2 && a.map_cols >= 2 && a.horizontal_scale > 0.f), "pulse_task_ref_state_init: bad height field");
        PULSE_REQUIRE(!a.heightsamples || (a.center_points && a.num_center_points >= 1 && a.num_center_points <= kTrLanes),
                      "pulse_task_ref_state_init: TERRAIN needs the centre grid (1 .. 32 points)");
    }
    unsigned blocks;
    if (const int rc = lane_group_blocks("pulse_task_ref_state_init", a.num_envs, kTrEnvs, blocks)) return rc;
    hipLaunchKernelGGL(task_reset_kernel, dim3(blocks), dim3(kTrThreads), 0, as_stream(s), a);
    return check_launch("pulse_task_ref_state_init");
}
