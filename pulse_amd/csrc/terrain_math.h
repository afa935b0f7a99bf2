// The only height-field lookup, shared by the kernels that stand on the terrain (traj_step.hip, crowd_obs.hip, task_reset.hip):
// Terrain.world_points_to_map / sample_height_points (phc/env/tasks/humanoid_pedestrian_terrain.py:1191-1270) and get_center_heights
// (:690-716, quat_apply_yaw): its yaw-only rotation for all three, its workgroup-wide mean for the two height-block kernels.
// Compile with -ffp-contract=off.
#pragma once
#include <cstdint>
#include "rot_math.h"

namespace pulse {

// isaacgym.torch_utils.quat_apply (3P): b + w t + xyz x t, t = 2 xyz x b
__device__ __forceinline__ V3 q_apply(const Q4 a, const V3 b) {
    const V3 t{(a.y * b.z - a.z * b.y) * 2.0f, (a.z * b.x - a.x * b.z) * 2.0f, (a.x * b.y - a.y * b.x) * 2.0f};
    return V3{b.x + a.w * t.x + (a.y * t.z - a.z * t.y), b.y + a.w * t.y + (a.z * t.x - a.x * t.z), b.z + a.w * t.z + (a.x * t.y - a.y * t.x)};
}

// the int16 height samples (rows x cols cells of horizontal_scale metres, vertical_scale metres per count)
struct HeightField { const int16_t* samples; int32_t rows, cols; float horizontal_scale, vertical_scale; };

template <typename Args>
__device__ __forceinline__ HeightField height_field_of(const Args& a) {
    return HeightField{a.heightsamples, a.map_rows, a.map_cols, a.horizontal_scale, a.vertical_scale};
}

// world_points_to_map: (points / horizontal_scale).long() truncates toward zero, then clip to [0, size - 2]; the two cells get_heights compares
__device__ __forceinline__ void height_cells(const HeightField& f, float wx, float wy, long long& c1, long long& c2) {
    long long px = (long long)(wx / f.horizontal_scale), py = (long long)(wy / f.horizontal_scale);
    px = px < 0 ? 0 : (px > f.rows - 2 ? f.rows - 2 : px);
    py = py < 0 ? 0 : (py > f.cols - 2 ? f.cols - 2 : py);
    c1 = px * f.cols + py;
    c2 = (px + 1) * f.cols + py + 1;
}
__device__ __forceinline__ float sample_height(const HeightField& f, float wx, float wy) {
    long long c1, c2;
    height_cells(f, wx, wy, c1, c2);
    const short h1 = f.samples[c1], h2 = f.samples[c2];
    return (float)(h1 < h2 ? h1 : h2) * f.vertical_scale;
}

// quat_apply_yaw's quaternion (:1572-1576): x = y = 0, then normalize
__device__ __forceinline__ Q4 yaw_quat(const Q4 q) {
    const float n = fmaxf(sqrtf(q.z * q.z + q.w * q.w), 1e-9f);
    return Q4{0.0f / n, 0.0f / n, q.z / n, q.w / n};
}

// The height a height block is measured from, for one env by its WHOLE workgroup (barriers inside: every thread calls it, at most 256 centre
// points).  use_center: get_center_heights -- the centre grid under the root, turned by the root's yaw only, one thread per point (their
// dependent gathers overlap), summed by thread 0 in the reference's order, mean; always the plain field, never a stamped one.  Otherwise
// the root's own height, and the second barrier is still crossed.
__device__ __forceinline__ float height_reference(const HeightField& f, bool use_center, const float* center_points, int num_center_points,
                                                  const Q4 root_q, const V3 root_p) {
    __shared__ float s_center;
    __shared__ float s_cpt[256];
    const int tid = threadIdx.x;
    if (use_center) {
        if (tid < num_center_points) {
            const V3 w = q_apply(yaw_quat(root_q), V3{center_points[2 * tid], center_points[2 * tid + 1], 0.0f});
            s_cpt[tid] = sample_height(f, w.x + root_p.x, w.y + root_p.y);
        }
        __syncthreads();
        if (tid == 0) {
            float sum = 0.0f;
            for (int c = 0; c < num_center_points; ++c) sum += s_cpt[c];
            s_center = sum / (float)num_center_points;
        }
    }
    __syncthreads();
    return use_center ? s_center : root_p.z;
}

}  // namespace pulse
