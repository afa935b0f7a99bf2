// poselib's quaternion algebra (poselib/core/rotation3d.py) and the scipy Rotation calls the conversion scripts make, in fp32, terms in the
// reference's order, and the clip lookup of a packed table: shared by the kernels that stand for poselib / scipy calls on whole clips
// (motion_build.hip, motion_ingest.hip, motion_smooth.hip, motion_export.hip).
// Compile with -ffp-contract=off.
#pragma once
#include "body_lanes.h"

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

// scipy's Rotation(q): q / sqrt(q . q)
__device__ __forceinline__ Q4 qunit_scipy(const Q4 q) {
    const float n = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    return Q4{q.x / n, q.y / n, q.z / n, q.w / n};
}
// scipy _compose_quat: p * q, the sign kept
__device__ __forceinline__ Q4 qcompose_scipy(const Q4 p, const Q4 q) {
    const float cx = p.y * q.z - p.z * q.y, cy = p.z * q.x - p.x * q.z, cz = p.x * q.y - p.y * q.x;
    Q4 r;
    r.x = p.w * q.x + q.w * p.x + cx;
    r.y = p.w * q.y + q.w * p.y + cy;
    r.z = p.w * q.z + q.w * p.z + cz;
    r.w = p.w * q.w - p.x * q.x - p.y * q.y - p.z * q.z;
    return r;
}

// scipy Rotation.from_rotvec (_rotation.pyx): xyzw, Taylor series of sin(angle / 2) / angle at angle <= 1e-3, w = cos(angle / 2) as it comes
__device__ __forceinline__ Q4 rotvec_to_quat(const float x, const float y, const float z) {
    const float angle = sqrtf(x * x + y * y + z * z);
    float scale;
    if ((double)angle <= 1e-3) {
        const float a2 = angle * angle;
        scale = 0.5f - a2 / 48.0f + a2 * a2 / 3840.0f;
    } else {
        scale = sinf(angle / 2.0f) / angle;
    }
    return Q4{scale * x, scale * y, scale * z, cosf(angle / 2.0f)};
}
// scipy Rotation.as_rotvec (_rotation.pyx) of Rotation.from_quat(q): normalise, w made >= 0, angle = 2 atan2(|xyz|, w), the Taylor series of
// angle / sin(angle / 2) at angle <= 1e-3
__device__ __forceinline__ V3 quat_to_rotvec_scipy(Q4 q) {
    q = qunit_scipy(q);
    if (q.w < 0.0f) q = Q4{-q.x, -q.y, -q.z, -q.w};
    const float angle = 2.0f * atan2f(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z), q.w);
    float scale;
    if ((double)angle <= 1e-3) {
        const float a2 = angle * angle;
        scale = 2.0f + a2 / 12.0f + 7.0f * a2 * a2 / 2880.0f;
    } else {
        scale = angle / sinf(angle / 2.0f);
    }
    return V3{scale * q.x, scale * q.y, scale * q.z};
}
// quat_to_exp_map (phc/utils/torch_utils.py:81-97): angle * axis of quat_to_angle_axis
__device__ __forceinline__ V3 q_to_exp_map(const Q4 q) {
    V3 ax;
    const float ang = q_to_angle_axis(q, &ax);
    return V3{ang * ax.x, ang * ax.y, ang * ax.z};
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
