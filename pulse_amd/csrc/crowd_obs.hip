// Crowd variant of the terrain task (HumanoidPedestrianTerrain with divide_group) for gfx950: the neighbour observation, people stamped
// into the height map, and the per-agent velocity channels of the height block.
//
// Replaces
//   compute_group_observation                            phc/env/tasks/humanoid_pedestrian_terrain.py:1700-1753
//   get_heights (root points, velocity_map)              :718-772
//   init_root_points                                     :643-660
//   Terrain.sample_height_points (groups / velocities)   :1200-1276
//   _compute_task_obs (tail: centre height, clip, scale) :414-437
//
// Three kernel shapes.  The neighbour search is one WAVE per env: its 64 lanes stride over the members of the env's group and six rounds of
// a wave arg-min (cross-lane shuffles, no LDS) pick the six nearest in order; the 165 output floats are then written as a coalesced row.
// The stamp is one thread per (person, root point) with an atomicMax into a per-group int32 OWNER grid (0 = empty, else env index + 1):
// the height field is never replicated per group, and the cells a stamp touched are listed so the next stamp clears exactly those.
// The height block is one 256-thread workgroup per env, as in traj_step.hip, reading the shared int16 field plus the group's owner grid;
// cell lookup and centre height are terrain_math.h's, the ones traj_step.hip uses.
// -ffp-contract=off: the expressions follow the reference's operation order.
#include "common.h"
#include "env_select.h"
#include "terrain_math.h"

namespace pulse {

__device__ const int kCrowdJoints[PULSE_CROWD_JOINTS] = {0, 1, 5, 9, 3, 7, 16, 21, 18, 23};

// ---- compute_group_observation: one wave per env, four envs per workgroup ---------------------------------------------------------------
__global__ void __launch_bounds__(256) crowd_group_obs_kernel(const pulse_crowd_group_obs_args a) {
    int64_t e;
    if (!select_env(a, blockIdx.x * 4 + (threadIdx.x >> 6), e)) return;                  // (whole waves leave: no barrier below)
    const int lane = threadIdx.x & 63;
    const int G = a.group_size;
    const int64_t g0 = (e / G) * G;                                                      // first env of the group: neighbours never leave [g0, g0 + G)
    const float* rb = a.rb + e * a.rb_env_stride;
    const V3 root_p{rb[0], rb[1], rb[2]};

    // six rounds: the smallest (distance, member) pair above the one picked before.  Round 0 is the env itself (distance 0) and is dropped,
    // as topk_idx[..., 1:] does; lane r - 1 keeps the pick of round r.
    float prev_d = -1.0f; int prev_m = -1;
    float sel_d = 0.0f; int sel_m = -1;
    for (int r = 0; r <= PULSE_CROWD_TOPK; ++r) {
        float best_d = INFINITY; int best_m = 0x7fffffff;
        for (int m = lane; m < G; m += 64) {
            const float* o = a.rb + (g0 + m) * a.rb_env_stride;
            const float dx = root_p.x - o[0], dy = root_p.y - o[1], dz = root_p.z - o[2];
            const float d = sqrtf(dx * dx + dy * dy + dz * dz);                          // torch.norm(..., dim=-1)
            const bool after = d > prev_d || (d == prev_d && m > prev_m);
            if (after && (d < best_d || (d == best_d && m < best_m))) { best_d = d; best_m = m; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float od = __shfl_xor(best_d, o, 64);
            const int om = __shfl_xor(best_m, o, 64);
            if (od < best_d || (od == best_d && om < best_m)) { best_d = od; best_m = om; }
        }
        prev_d = best_d; prev_m = best_m;
        if (r >= 1 && lane == r - 1) { sel_d = best_d; sel_m = best_m; }
    }

    const Q4 hinv = heading_quat(remove_base_rot(Q4{rb[3], rb[4], rb[5], rb[6]}, a.upright_start), true);
    float* out = a.obs + e * a.obs_stride + a.obs_offset;
    for (int o = lane; o < PULSE_CROWD_GROUP_OBS; o += 64) {
        const bool is_vel = o >= PULSE_CROWD_TOPK * PULSE_CROWD_JOINTS * 3;
        const int q = is_vel ? o - PULSE_CROWD_TOPK * PULSE_CROWD_JOINTS * 3 : o;
        const int k = is_vel ? q / 3 : q / (PULSE_CROWD_JOINTS * 3);
        const int j = is_vel ? 0 : (q / 3) % PULSE_CROWD_JOINTS;
        const int c = q % 3;
        const int m = __shfl(sel_m, k, 64);
        const float d = __shfl(sel_d, k, 64);
        float val = 0.0f;
        if (m >= 0 && m < G && !(d > 10.0f)) {                                           // (an unpicked slot -- NaN distances -- stays zero and is never read)
            const float* nb = a.rb + (g0 + m) * a.rb_env_stride;
            V3 v;
            if (is_vel) v = V3{nb[7], nb[8], nb[9]};
            else { const float* b = nb + 13 * kCrowdJoints[j]; v = V3{b[0] - root_p.x, b[1] - root_p.y, b[2] - root_p.z}; }
            const V3 l = qrot(hinv, v);
            val = c == 0 ? l.x : (c == 1 ? l.y : l.z);
        }
        out[o] = val;
    }
}

// ---- stamps ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) crowd_clear_kernel(const pulse_crowd_stamp_args a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)a.num_envs * PULSE_CROWD_ROOT_POINTS) return;
    const int64_t e = t / PULSE_CROWD_ROOT_POINTS;
    const int64_t plane = (int64_t)a.map_rows * a.map_cols;
    const int c = a.cells[t];
    if (c >= 0 && c < plane) a.owner[(e / a.group_size) * plane + c] = 0;
}

__global__ void __launch_bounds__(256) crowd_stamp_kernel(const pulse_crowd_stamp_args a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)a.num_envs * PULSE_CROWD_ROOT_POINTS) return;
    const int64_t e = t / PULSE_CROWD_ROOT_POINTS;
    const int r = (int)(t - e * PULSE_CROWD_ROOT_POINTS);
    const int ix = r / 20, iy = r % 20;
    // init_root_points: np.linspace in float64 (start + i * step, the last point set to the stop), assigned into a float32 tensor
    const float lx = ix == 9 ? 0.25f : (float)((double)ix * (0.5 / 9.0) + -0.25);
    const float ly = iy == 19 ? 0.5f : (float)((double)iy * (1.0 / 19.0) + -0.5);
    const float* rb = a.rb + e * a.rb_env_stride;
    const Q4 hq = heading_quat(Q4{rb[3], rb[4], rb[5], rb[6]}, false);                    // the RAW root rotation (get_heights :750)
    const V3 w = q_apply(hq, V3{lx, ly, 0.0f});
    long long c1, c2;
    height_cells(HeightField{nullptr, a.map_rows, a.map_cols, a.horizontal_scale, 0.0f}, w.x + rb[0], w.y + rb[1], c1, c2);   // (cells only: no samples read)
    const int cell = (int)c1;
    const int64_t plane = (int64_t)a.map_rows * a.map_cols;
    atomicMax(a.owner + (e / a.group_size) * plane + cell, (int)e + 1);
    a.cells[t] = cell;
}

// ---- the height block: one workgroup per env -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) crowd_height_kernel(const pulse_crowd_heights_args a) {
    int64_t e;
    if (!select_env(a, blockIdx.x, e)) return;                                           // (the whole workgroup leaves)
    const int tid = threadIdx.x;
    const float* rb = a.rb + e * a.rb_env_stride;
    const V3 root_p{rb[0], rb[1], rb[2]};
    const Q4 raw_q{rb[3], rb[4], rb[5], rb[6]};
    const HeightField hf = height_field_of(a);
    const int64_t plane = (int64_t)a.map_rows * a.map_cols;
    const int32_t* ow = a.owner ? a.owner + (e / a.group_size) * plane : nullptr;
    const float ref = height_reference(hf, a.use_center_height, a.center_points, a.num_center_points, remove_base_rot(raw_q, a.upright_start), root_p);

    const float* sb = rb + 13 * a.sensor_body;
    const Q4 hq = heading_quat(remove_base_rot(Q4{sb[3], sb[4], sb[5], sb[6]}, a.upright_start), false);
    // velocities: the env's own root velocity and calc_heading_quat_inv of its RAW root rotation (sample_height_points :1219-1221, 1270-1272)
    const V3 own_v{rb[7], rb[8], rb[9]};
    const Q4 vinv = a.velocity_map ? heading_quat(raw_q, true) : Q4{0.f, 0.f, 0.f, 1.f};
    const int ch = a.velocity_map ? 3 : 1;
    float* ho = a.obs + e * a.obs_stride + a.obs_offset;
    // One point per thread and pass, with the owner grid read beside the field.  traj_step.hip's loop over the same points takes four per
    // thread with their gathers batched and knows no owners: two kernels on purpose, one set of cells (height_cells).
    for (int p = tid; p < a.num_height_points; p += 256) {
        const V3 w = q_apply(hq, V3{a.height_points[2 * p], a.height_points[2 * p + 1], 0.0f});
        long long c1, c2;
        height_cells(hf, w.x + sb[0], w.y + sb[1], c1, c2);
        int h1 = a.heightsamples[c1], h2 = a.heightsamples[c2];
        int o1 = 0;
        if (ow) {
            o1 = ow[c1];
            if (o1 != 0) h1 += a.stamp_raise;
            if (ow[c2] != 0) h2 += a.stamp_raise;
        }
        const float h = (float)(h1 < h2 ? h1 : h2) * a.vertical_scale;
        ho[ch * p] = fminf(fmaxf(ref - h, -3.0f), 3.0f) * a.height_meas_scale;
        if (a.velocity_map) {
            V3 v{0.0f, 0.0f, 0.0f};
            if (o1 > 0 && o1 <= a.num_envs) { const float* ob = a.rb + (int64_t)(o1 - 1) * a.rb_env_stride; v = V3{ob[7], ob[8], ob[9]}; }
            float vx, vy;
            if (ow) {
                const V3 l = qrot(vinv, V3{v.x - own_v.x, v.y - own_v.y, v.z - own_v.z});
                vx = l.x; vy = l.y;
            } else {
                const V3 ego = qrot(vinv, own_v);
                vx = 0.0f - ego.x; vy = 0.0f - ego.y;
            }
            if (!a.use_center_height) { vx = root_p.z - vx; vy = root_p.z - vy; }        // the root-height branch subtracts on every channel (:427)
            ho[3 * p + 1] = fminf(fmaxf(vx, -3.0f), 3.0f) * a.height_meas_scale;
            ho[3 * p + 2] = fminf(fmaxf(vy, -3.0f), 3.0f) * a.height_meas_scale;
        }
    }
}

}  // namespace pulse

using namespace pulse;

extern "C" {

int pulse_sizeof_crowd_group_obs_args(void) { return (int)sizeof(pulse_crowd_group_obs_args); }
int pulse_sizeof_crowd_stamp_args(void) { return (int)sizeof(pulse_crowd_stamp_args); }
int pulse_sizeof_crowd_heights_args(void) { return (int)sizeof(pulse_crowd_heights_args); }

int pulse_crowd_group_obs(const pulse_crowd_group_obs_args* args, pulse_stream_t s) {
    PULSE_REQUIRE(args != nullptr, "pulse_crowd_group_obs: null args");
    const pulse_crowd_group_obs_args& a = *args;
    PULSE_REQUIRE(a.num_envs >= 0, "pulse_crowd_group_obs: negative num_envs");
    PULSE_REQUIRE(a.group_size >= PULSE_CROWD_TOPK + 1, "pulse_crowd_group_obs: group_size %d < 6 (the reference's topk of 6 distances, "
                  "humanoid_pedestrian_terrain.py:1724)", a.group_size);
    PULSE_REQUIRE(a.num_envs % a.group_size == 0, "pulse_crowd_group_obs: num_envs %d is not a multiple of group_size %d", a.num_envs, a.group_size);
    const int count = env_count(a);
    PULSE_REQUIRE(count >= 0, "pulse_crowd_group_obs: negative num_ids");
    if (count == 0) return PULSE_OK;
    PULSE_REQUIRE(a.rb && a.num_bodies >= 24 && a.rb_env_stride >= 13LL * a.num_bodies,
                  "pulse_crowd_group_obs: bad rigid-body state (24 or more bodies of 13 floats: the selected bodies reach index 23)");
    PULSE_REQUIRE(a.obs && a.obs_offset >= 0 && a.obs_stride >= (int64_t)a.obs_offset + PULSE_CROWD_GROUP_OBS, "pulse_crowd_group_obs: bad obs target");
    hipLaunchKernelGGL(crowd_group_obs_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, as_stream(s), a);
    return check_launch("pulse_crowd_group_obs");
}

int pulse_crowd_stamp(const pulse_crowd_stamp_args* args, pulse_stream_t s) {
    PULSE_REQUIRE(args != nullptr, "pulse_crowd_stamp: null args");
    const pulse_crowd_stamp_args& a = *args;
    PULSE_REQUIRE(a.num_envs >= 0, "pulse_crowd_stamp: negative num_envs");
    PULSE_REQUIRE(a.group_size >= 1, "pulse_crowd_stamp: group_size %d < 1", a.group_size);
    PULSE_REQUIRE(a.num_envs % a.group_size == 0, "pulse_crowd_stamp: num_envs %d is not a multiple of group_size %d", a.num_envs, a.group_size);
    if (a.num_envs == 0) return PULSE_OK;
    PULSE_REQUIRE(a.rb && a.rb_env_stride >= 13, "pulse_crowd_stamp: bad rigid-body state");
    PULSE_REQUIRE(a.map_rows >= 2 && a.map_cols >= 2 && (int64_t)a.map_rows * a.map_cols < (1LL << 31) && a.horizontal_scale > 0.f,
                  "pulse_crowd_stamp: bad height field");
    PULSE_REQUIRE(a.owner && a.cells, "pulse_crowd_stamp: null owner grid / cell list");
    const int64_t total = (int64_t)a.num_envs * PULSE_CROWD_ROOT_POINTS;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (a.clear) hipLaunchKernelGGL(crowd_clear_kernel, grid, dim3(256), 0, as_stream(s), a);
    hipLaunchKernelGGL(crowd_stamp_kernel, grid, dim3(256), 0, as_stream(s), a);
    return check_launch("pulse_crowd_stamp");
}

int pulse_crowd_heights(const pulse_crowd_heights_args* args, pulse_stream_t s) {
    PULSE_REQUIRE(args != nullptr, "pulse_crowd_heights: null args");
    const pulse_crowd_heights_args& a = *args;
    PULSE_REQUIRE(a.num_envs >= 0, "pulse_crowd_heights: negative num_envs");
    if (a.owner) {
        PULSE_REQUIRE(a.group_size >= 1, "pulse_crowd_heights: group_size %d < 1", a.group_size);
        PULSE_REQUIRE(a.num_envs % a.group_size == 0, "pulse_crowd_heights: num_envs %d is not a multiple of group_size %d", a.num_envs, a.group_size);
    }
    const int count = env_count(a);
    PULSE_REQUIRE(count >= 0, "pulse_crowd_heights: negative num_ids");
    if (count == 0) return PULSE_OK;
    PULSE_REQUIRE(a.rb && a.num_bodies >= 1 && a.rb_env_stride >= 13LL * a.num_bodies, "pulse_crowd_heights: bad rigid-body state");
    PULSE_REQUIRE(a.heightsamples && a.map_rows >= 2 && a.map_cols >= 2 && a.horizontal_scale > 0.f, "pulse_crowd_heights: bad height field");
    PULSE_REQUIRE(a.height_points && a.num_height_points >= 1 && a.sensor_body >= 0 && a.sensor_body < a.num_bodies,
                  "pulse_crowd_heights: height sensor needs its grid and a body");
    PULSE_REQUIRE(!a.use_center_height || (a.center_points && a.num_center_points >= 1 && a.num_center_points <= 256),
                  "pulse_crowd_heights: use_center_height needs the centre grid (1 .. 256 points)");
    const int64_t width = (int64_t)(a.velocity_map ? 3 : 1) * a.num_height_points;
    PULSE_REQUIRE(a.obs && a.obs_offset >= 0 && a.obs_stride >= a.obs_offset + width, "pulse_crowd_heights: bad obs target");
    hipLaunchKernelGGL(crowd_height_kernel, dim3((unsigned)count), dim3(256), 0, as_stream(s), a);
    return check_launch("pulse_crowd_heights");
}
}
