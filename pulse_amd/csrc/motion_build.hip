// Building the packed reference-motion records from raw clips on gfx950: what MotionLibSMPL.load_motion_with_skeleton
// (phc/utils/motion_lib_smpl.py:101-174, the mesh_parsers-is-None path) computes clip by clip with poselib, np.gradient and
// scipy's Gaussian filter in up to 64 worker processes -- here two launches over every resident clip at once, straight into
// the records motion_state.hip reads (include/pulse_hip.h section 2b').
//
// Pass 1, per frame (a 32-lane half-wave per frame up to 32 bodies, a whole wave for 33 .. 64; lane j <-> body j):
//   heading rotation (fp64, as scipy applies it) -> grs; lrs = quat_mul_norm(conj(g[parent]), g[b]) from the rotations of the frame
//   parked in LDS; forward kinematics level by level down the tree through LDS (one barrier per tree level: a chain of J - 1 bodies
//   takes J - 1 rounds, a star one) -> gts; padding columns zeroed.
// Pass 2, per 16 consecutive records x every body: the unfiltered linear / angular velocities of the 16 + 2 x 8 records around the
//   tile go to LDS (each computed inside its OWN clip: np.gradient's one-sided ends, identity at the last frame), then 17 taps with
//   the tap index clamped to the clip of the output record -- a clamped tap moves towards the output record, so it stays inside the
//   tile and never crosses into a neighbouring clip of the packed table; dvs from lrs of the record and its successor.
// Memory bound: J x 16 + 12 bytes per frame read from the staging buffers and 4 x frame_stride bytes written per frame; pass 2
// re-reads grs / lrs / gts of pass 1 (twice over with the halo).  Measured: profiles/motion_build.txt.
// Compiled with -ffp-contract=off: the operation order of the reference's fp32 run.
#include "motion_math.h"
#include "poselib_math.h"

namespace pulse {

constexpr int kMbThreads = 256;
constexpr int kMbMaxBodies = 64;
constexpr int kMbRadius = 8;                      // gaussian_filter1d: int(truncate 4.0 * sigma 2 + 0.5)
constexpr int kMbTile = 16;                       // output records per block of pass 2
constexpr int kMbRows = kMbTile + 2 * kMbRadius;  // records whose unfiltered velocities a tile needs

// ---- pass 1: heading, grs, lrs, FK -> gts, padding ------------------------------------------------------------------------------------
template <int LB>
__global__ void __launch_bounds__(LaneGroup<LB>::threads) motion_build_frames_kernel(const pulse_motion_build_args a, const BodyTree<kMbMaxBodies> tree, const int pad_start) {
    constexpr int kSlots = LaneGroup<LB>::slots;
    __shared__ Q4 s_g[kSlots][LB];        // global rotations of the frame (after the heading rotation)
    __shared__ Q4 s_r[kSlots][LB];        // FK: rotation of the global transformation
    __shared__ V3 s_t[kSlots][LB];        // FK: translation of the global transformation
    const auto [slot, b, g] = lane_group<LB>();
    const int J = a.num_bodies;
    const bool live = g < a.total_frames && b < J;          // no early return: every thread reaches the barriers
    float* rec = nullptr;
    Q4 q{0.0f, 0.0f, 0.0f, 1.0f}, l = q;
    V3 lt{0.0f, 0.0f, 0.0f};
    if (live) {
        const int m = clip_of(a.clip_out_start, a.num_clips, g);
        const long long t = g - a.clip_out_start[m];
        long long src = a.clip_src_start[m] + (a.clip_crop_start ? a.clip_crop_start[m] : 0) + t;
        src = src < 0 ? 0 : (src > a.src_frames - 1 ? a.src_frames - 1 : src);          // a bad clip table reads a wrong frame, never out of bounds
        rec = a.frames + g * a.frame_stride;
        q = load_q4(a.src_rot + (src * J + b) * 4);
        const float* tr = a.src_trans + 3 * src;
        lt = b == 0 ? V3{tr[0], tr[1], tr[2]} : V3{a.local_translation[((long long)m * J + b) * 3], a.local_translation[((long long)m * J + b) * 3 + 1],
                                                   a.local_translation[((long long)m * J + b) * 3 + 2]};
        if (a.clip_heading) {
            // random_heading_rot * sRot.from_quat(q) and trans @ R^T (motion_lib_smpl.py:134-139): scipy normalises q and works in double
            const double h = (double)a.clip_heading[m];
            const double sz = sin(0.5 * h), cw = cos(0.5 * h);
            double x = q.x, y = q.y, z = q.z, w = q.w;
            const double n = sqrt(x * x + y * y + z * z + w * w);
            x /= n; y /= n; z /= n; w /= n;
            q = Q4{(float)(cw * x - sz * y), (float)(cw * y + sz * x), (float)(cw * z + sz * w), (float)(cw * w - sz * z)};
            if (b == 0) {
                const double c = cos(h), s = sin(h);
                const double tx = lt.x, ty = lt.y;
                lt.x = (float)(c * tx - s * ty);
                lt.y = (float)(s * tx + c * ty);
            }
        }
        store_q4(rec + a.off_grs + 4 * b, q);
        for (int c = pad_start + b; c < a.frame_stride; c += J) rec[c] = 0.0f;
    }
    s_g[slot][b] = q;
    __syncthreads();
    const int p = b < J ? tree.parent[b] : -1;
    if (live) {
        l = p < 0 ? q : qmul_norm(qconj(s_g[slot][p]), q);
        store_q4(rec + a.off_lrs + 4 * b, l);
    }
    // FK, one tree level per round: transform_mul(global[parent], local[b]) (rotation3d.py:318-326)
    const int depth = b < J ? tree.depth[b] : -1;
    for (int lvl = 0; lvl <= tree.max_depth; ++lvl) {
        if (depth == lvl) {
            Q4 R = l;
            V3 T = lt;
            if (p >= 0) {
                const Q4 Rp = s_r[slot][p];
                const V3 Tp = s_t[slot][p], rv = qrotate_plain(Rp, lt);
                R = qmul_norm(Rp, l);
                T = V3{rv.x + Tp.x, rv.y + Tp.y, rv.z + Tp.z};
            }
            s_r[slot][b] = R;
            s_t[slot][b] = T;
            if (live) { float* o = rec + a.off_gts + 3 * b; o[0] = T.x; o[1] = T.y; o[2] = T.z; }
        }
        __syncthreads();
    }
}

// ---- pass 2: gvs, gavs (np.gradient / quaternion difference -> 17-tap Gaussian), dvs ---------------------------------------------------
__global__ void __launch_bounds__(kMbThreads) motion_build_velocity_kernel(const pulse_motion_build_args a) {
    __shared__ float s_raw[kMbRows][kMbMaxBodies][6];       // unfiltered [linear | angular] velocity of (row, body)
    __shared__ long long s_lo[kMbRows], s_hi[kMbRows];      // first / last record of the row's clip
    __shared__ float s_dt[kMbRows];
    const int J = a.num_bodies;
    const long long g0 = (long long)blockIdx.x * kMbTile - kMbRadius;        // record of row 0
    if (threadIdx.x < kMbRows) {
        const long long g = g0 + threadIdx.x;
        long long lo = 0, hi = -1;
        float dt = 1.0f;
        if (g >= 0 && g < a.total_frames) {
            const int m = clip_of(a.clip_out_start, a.num_clips, g);
            lo = a.clip_out_start[m];
            hi = a.clip_out_start[m + 1] - 1;
            lo = lo < 0 ? 0 : lo;                                            // a bad clip table gives wrong values, never an access outside the records
            hi = hi > a.total_frames - 1 ? a.total_frames - 1 : hi;
            dt = a.clip_dt[m];
        }
        s_lo[threadIdx.x] = lo; s_hi[threadIdx.x] = hi; s_dt[threadIdx.x] = dt;
    }
    __syncthreads();
    for (int w = threadIdx.x; w < kMbRows * J; w += kMbThreads) {
        const int r = w / J, b = w % J;
        const long long g = g0 + r, lo = s_lo[r], hi = s_hi[r];
        float* raw = s_raw[r][b];
        if (hi < lo + 1 || g < lo || g > hi) {               // outside the table (or a clip of one frame, which the launcher refuses)
            for (int c = 0; c < 6; ++c) raw[c] = 0.0f;
            continue;
        }
        const float dt = s_dt[r];
        const float* rec = a.frames + g * a.frame_stride;
        // np.gradient: central differences inside ((f[t+1] - f[t-1]) / 2), first differences at both ends
        const long long gp = g > lo ? g - 1 : g, gn = g < hi ? g + 1 : g;
        const float* pp = a.frames + gp * a.frame_stride + a.off_gts + 3 * b;
        const float* pn = a.frames + gn * a.frame_stride + a.off_gts + 3 * b;
        const float den = (g > lo && g < hi) ? 2.0f : 1.0f;
        for (int c = 0; c < 3; ++c) raw[c] = ((pn[c] - pp[c]) / den) / dt;
        // quat_mul_norm(r[t+1], inverse(r[t])), identity at the clip's last frame; quat_angle_axis (rotation3d.py:231-240)
        Q4 d{0.0f, 0.0f, 0.0f, 1.0f};
        if (g < hi) d = qmul_plain(load_q4(rec + a.frame_stride + a.off_grs + 4 * b), qconj(load_q4(rec + a.off_grs + 4 * b)));
        d = qnormalize_pos(d);
        const float s = 2.0f * (d.w * d.w) - 1.0f;
        const float angle = acosf(fminf(fmaxf(s, -1.0f), 1.0f));
        const float n = fmaxf(sqrtf(d.x * d.x + d.y * d.y + d.z * d.z), 1e-9f);
        raw[3] = ((d.x / n) * angle) / dt;
        raw[4] = ((d.y / n) * angle) / dt;
        raw[5] = ((d.z / n) * angle) / dt;
    }
    __syncthreads();
    for (int w = threadIdx.x; w < kMbTile * J; w += kMbThreads) {
        const int i = w / J, b = w % J, r = i + kMbRadius;
        const long long g = g0 + r, lo = s_lo[r], hi = s_hi[r];
        if (hi < lo + 1 || g < lo || g > hi) continue;
        float* rec = a.frames + g * a.frame_stride;
        // scipy correlate1d, symmetric filter: centre tap, then the pairs from the outermost inwards; mode "nearest" clamps to the clip
        float acc[6];
        for (int c = 0; c < 6; ++c) acc[c] = s_raw[r][b][c] * a.filter_w[0];
        for (int k = kMbRadius; k >= 1; --k) {
            const long long gl = g - k < lo ? lo : g - k, gh = g + k > hi ? hi : g + k;
            const float* xl = s_raw[(int)(gl - g0)][b];
            const float* xh = s_raw[(int)(gh - g0)][b];
            for (int c = 0; c < 6; ++c) acc[c] = acc[c] + (xl[c] + xh[c]) * a.filter_w[k];
        }
        float* ov = rec + a.off_gvs + 3 * b;
        float* ow = rec + a.off_gavs + 3 * b;
        for (int c = 0; c < 3; ++c) { ov[c] = acc[c]; ow[c] = acc[3 + c]; }
        if (b >= 1) {
            // local_rotation_to_dof_vel (motion_lib_base.py:47-53) of frames (t, t + 1); the last frame repeats the one before it (:67)
            const long long gt = g < hi ? g : hi - 1;
            const float* r0 = a.frames + gt * a.frame_stride + a.off_lrs + 4 * b;
            const Q4 dq = qmul(qconj(load_q4(r0)), load_q4(r0 + a.frame_stride));
            V3 ax;
            const float ang = q_to_angle_axis(dq, &ax);
            const float dt = s_dt[r];
            float* od = rec + a.off_dvs + 3 * (b - 1);
            od[0] = (ax.x * ang) / dt; od[1] = (ax.y * ang) / dt; od[2] = (ax.z * ang) / dt;
        }
    }
}

}  // namespace pulse

extern "C" int pulse_sizeof_motion_build_args(void) { return (int)sizeof(pulse_motion_build_args); }

extern "C" int pulse_motion_build(const pulse_motion_build_args* args, pulse_stream_t s) {
    using namespace pulse;
    PULSE_REQUIRE(args != nullptr, "pulse_motion_build: null args");
    const pulse_motion_build_args& a = *args;
    PULSE_REQUIRE(a.num_clips >= 0 && a.total_frames >= 0, "pulse_motion_build: negative clip / frame count");
    if (a.num_clips == 0 && a.total_frames == 0) return PULSE_OK;
    const int J = a.num_bodies;
    PULSE_REQUIRE(J >= 1 && J <= kMbMaxBodies, "pulse_motion_build: num_bodies %d not in [1,64]", J);
    PULSE_REQUIRE(a.src_rot && a.src_trans, "pulse_motion_build: null staging pointer (src_rot / src_trans)");
    PULSE_REQUIRE(a.clip_src_start && a.clip_out_start && a.clip_dt, "pulse_motion_build: null per-clip table (clip_src_start / clip_out_start / clip_dt)");
    PULSE_REQUIRE(a.clip_frames_host != nullptr, "pulse_motion_build: null clip_frames_host (the host copy of the frame counts)");
    PULSE_REQUIRE(a.local_translation != nullptr, "pulse_motion_build: null local_translation");
    PULSE_REQUIRE(a.frames != nullptr, "pulse_motion_build: null frames (the output records)");
    PULSE_REQUIRE(a.src_frames >= 1, "pulse_motion_build: src_frames %lld: the staging buffers are empty", (long long)a.src_frames);
    BodyTree<kMbMaxBodies> tree;
    if (const int rc = check_tree("pulse_motion_build", a.parent_indices_host, J, tree)) return rc;
    long long sum = 0;
    for (int m = 0; m < a.num_clips; ++m) {
        const long long f = a.clip_frames_host[m];
        PULSE_REQUIRE(f >= 2, "pulse_motion_build: clip %d has %lld frame(s): at least 2 are needed (np.gradient raises below 2)", m, f);
        sum += f;
    }
    PULSE_REQUIRE(sum == a.total_frames, "pulse_motion_build: the clips hold %lld frames but total_frames is %lld", sum, (long long)a.total_frames);
    if (const int rc = check_record_layout("pulse_motion_build", J, a.frame_stride, a.off_gts, a.off_grs, a.off_lrs, a.off_gvs, a.off_gavs, a.off_dvs, a.frames)) return rc;
    PULSE_REQUIRE(reinterpret_cast<uintptr_t>(a.src_rot) % 16 == 0, "pulse_motion_build: src_rot must be 16-byte aligned");
    const bool wide = J > kHalfWave;
    unsigned blocks1, blocks2;
    if (const int rc = lane_group_blocks("pulse_motion_build", a.total_frames, wide ? LaneGroup<64>::slots : LaneGroup<32>::slots, blocks1)) return rc;
    if (const int rc = lane_group_blocks("pulse_motion_build", a.total_frames, kMbTile, blocks2)) return rc;
    const int used = 20 * J - 3;                            // the padding columns start behind the six fields
    if (wide) hipLaunchKernelGGL(motion_build_frames_kernel<64>, dim3(blocks1), dim3(LaneGroup<64>::threads), 0, as_stream(s), a, tree, used);
    else hipLaunchKernelGGL(motion_build_frames_kernel<32>, dim3(blocks1), dim3(LaneGroup<32>::threads), 0, as_stream(s), a, tree, used);
    const int rc = check_launch("pulse_motion_build (frames)");
    if (rc != PULSE_OK) return rc;
    hipLaunchKernelGGL(motion_build_velocity_kernel, dim3(blocks2), dim3(kMbThreads), 0, as_stream(s), a);
    return check_launch("pulse_motion_build (velocities)");
}
