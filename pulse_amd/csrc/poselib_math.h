// poselib's quaternion algebra (poselib/core/rotation3d.py) in fp32, terms in the reference's order, and the clip lookup of a packed
// table: shared by the kernels that stand for poselib calls on whole clips (motion_build.hip, motion_ingest.hip).
// Compile with -ffp-contract=off.
#pragma once
#include "common.h"
#include "rot_math.h"

namespace pulse {

// poselib rotation3d.quat_mul (:15-27): the plain 16-multiply product, terms in the reference's order
__device__ __forceinline__ Q4 qmul_plain(const Q4 a, const Q4 b) {
    Q4 r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return r;
}
// quat_normalize = quat_unit(quat_pos(q)) (:31-38, 51-56, 93-98)
__device__ __forceinline__ Q4 qnormalize_pos(Q4 q) {
    const float s = q.w < 0.0f ? -1.0f : 1.0f;                       // (1 - 2 z), z = (w < 0)
    q = Q4{s * q.x, s * q.y, s * q.z, s * q.w};
    const float n = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-9f);
    return Q4{q.x / n, q.y / n, q.z / n, q.w / n};
}
__device__ __forceinline__ Q4 qmul_norm(const Q4 a, const Q4 b) { return qnormalize_pos(qmul_plain(a, b)); }
// quat_rotate (:206-211): imaginary part of (q (v, 0)) conj(q)
__device__ __forceinline__ V3 qrotate_plain(const Q4 q, const V3 v) {
    const Q4 t = qmul_plain(qmul_plain(q, Q4{v.x, v.y, v.z, 0.0f}), qconj(q));
    return V3{t.x, t.y, t.z};
}

// clip of packed record g: the last m with clip_out_start[m] <= g (clip_out_start ascending, [M] = total)
__device__ __forceinline__ int clip_of(const int64_t* starts, int num_clips, long long g) {
    int lo = 0, hi = num_clips - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace pulse
