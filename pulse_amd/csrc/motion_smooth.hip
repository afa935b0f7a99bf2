// Generated (text-to-motion) SMPL motion -> the staging layout pulse_motion_ingest reads, and the smoothing the reference applies to what
// ingest makes of it (include/pulse_hip.h section 2b'.1a), on gfx950: what scripts/data_process/convert_data_mdm.py:48-61 and :128-141 compute
// clip by clip with scipy, scipy.ndimage and poselib on the CPU -- here over every frame of every clip of a packed buffer, no host read-back.
//
// pulse_motion_euler_pose (one launch): a 32-lane half-wave per frame, lane s <-> SMPL joint s (24 of 32 lanes), lanes 0 .. 2 also the
//   translation's components.  scipy evaluates from_euler / __mul__ / as_rotvec / as_matrix in DOUBLE whatever the dtype of the input, and the
//   angles come in degrees: so does this kernel, with one rounding to fp32 on the store (72 + 3 floats a frame; the trigonometry is free
//   beside the launch).
// pulse_motion_smooth (three launches):
//   1. sign bits.  Half-wave per frame, lane = body: the raw test of quat_correct between frame t - 1 and t of the same clip
//      (|a - b| > |a + b|, strict), one ballot per wave, its 64 bits split into the two frames' 32-bit words (bit b = body b; frame 0 of a clip: 0).
//   2. scan.  The corrected sign is the prefix XOR of the raw tests along the clip (negating frame t - 1 swaps the two norms of the test at t).
//      One wave per clip, lane = frame, 64 frames a step (shuffle-up XOR scan), the last lane's word carried into the next step; in place.
//   3. filter.  Half-wave per output frame, lane = body: 2 r + 1 taps of the sign-corrected globals read through the caches (neighbouring
//      frames share 2 r of them: no LDS tile, the taps of the eight frames of a workgroup are 8 + 2 r rows of 16 J bytes), tap index clamped to
//      the frame's own clip; scipy correlate1d's order for a symmetric kernel (centre, then the pairs from the outermost inwards) and its
//      DOUBLE accumulator, rounded to fp32 once; fp32 from there: / norm, SkeletonState.local_rotation from one parent-lane read.  Lanes 0 .. 2
//      filter the root translation the same way.
// Every lane of a wave reaches every cross-lane operation; lanes without a frame or body load and store nothing.  A bad clip table computes
// wrong values, never an address outside the buffers: clip bounds and tap indices are clamped to [0, total_frames).
// Compiled with -ffp-contract=off.  Measured: profiles/mdm_ingest.txt.
#include "poselib_math.h"

namespace pulse {

using MsGroup = LaneGroup<kHalfWave>;
constexpr int kMsJoints = PULSE_INGEST_SMPL_JOINTS, kMsMaxRadius = PULSE_SMOOTH_MAX_RADIUS;
constexpr int kMsScanThreads = 256, kMsScanClips = kMsScanThreads / kWave;     // a wave per clip

struct D4 { double x, y, z, w; };
// scipy _compose_quat in double
__device__ __forceinline__ D4 dcompose(const D4 p, const D4 q) {
    const double cx = p.y * q.z - p.z * q.y, cy = p.z * q.x - p.x * q.z, cz = p.x * q.y - p.y * q.x;
    return D4{p.w * q.x + q.w * p.x + cx, p.w * q.y + q.w * p.y + cy, p.w * q.z + q.w * p.z + cz, p.w * q.w - p.x * q.x - p.y * q.y - p.z * q.z};
}
// scipy Rotation.as_rotvec of a quaternion as it is held (no renormalisation): w made >= 0, angle = 2 atan2(|xyz|, w)
__device__ __forceinline__ void drotvec(D4 q, double out[3]) {
    if (q.w < 0.0) q = D4{-q.x, -q.y, -q.z, -q.w};
    const double angle = 2.0 * atan2(sqrt(q.x * q.x + q.y * q.y + q.z * q.z), q.w);
    double scale;
    if (angle <= 1e-3) {
        const double a2 = angle * angle;
        scale = 2.0 + a2 / 12.0 + 7.0 * a2 * a2 / 2880.0;
    } else {
        scale = angle / sin(angle / 2.0);
    }
    out[0] = scale * q.x; out[1] = scale * q.y; out[2] = scale * q.z;
}
// scipy Rotation.from_rotvec in double
__device__ __forceinline__ D4 dfrom_rotvec(const double v[3]) {
    const double angle = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    double scale;
    if (angle <= 1e-3) {
        const double a2 = angle * angle;
        scale = 0.5 - a2 / 48.0 + a2 * a2 / 3840.0;
    } else {
        scale = sin(angle / 2.0) / angle;
    }
    return D4{scale * v[0], scale * v[1], scale * v[2], cos(angle / 2.0)};
}

// first and last frame of the clip that holds packed frame g, inside [0, total)
__device__ __forceinline__ void clip_range(const int64_t* starts, int num_clips, long long total, long long g, long long& lo, long long& hi) {
    const int m = clip_of(starts, num_clips, g);
    lo = starts[m];
    hi = starts[m + 1] - 1;
    lo = lo < 0 ? 0 : (lo > g ? g : lo);
    hi = hi > total - 1 ? total - 1 : (hi < g ? g : hi);
}

__global__ void __launch_bounds__(MsGroup::threads) motion_euler_pose_kernel(const pulse_motion_euler_pose_args a) {
    const auto [slot, s, g] = lane_group<kHalfWave>();
    if (g >= a.total_frames) return;                       // no cross-lane operation in this kernel
    if (s < kMsJoints) {
        const float* e = a.src_theta + g * (3 * kMsJoints) + 3 * s;
        // from_euler('XYZ', degrees=True): deg2rad, the elementary quaternions composed left to right (intrinsic)
        const double k = 0.017453292519943295;             // pi / 180 as numpy's deg2rad holds it
        const double hx = (double)e[0] * k / 2.0, hy = (double)e[1] * k / 2.0, hz = (double)e[2] * k / 2.0;
        D4 q = dcompose(dcompose(D4{sin(hx), 0.0, 0.0, cos(hx)}, D4{0.0, sin(hy), 0.0, cos(hy)}), D4{0.0, 0.0, sin(hz), cos(hz)});
        double v[3];
        drotvec(q, v);
        if (s == 0) {                                      // (transform * from_rotvec(root)).as_rotvec(); __mul__ normalises its product
            const D4 t{a.root_quat[0], a.root_quat[1], a.root_quat[2], a.root_quat[3]};
            q = dcompose(t, dfrom_rotvec(v));
            const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
            drotvec(D4{q.x / n, q.y / n, q.z / n, q.w / n}, v);
        }
        float* o = a.out_pose + g * (3 * kMsJoints) + 3 * s;
        o[0] = (float)v[0]; o[1] = (float)v[1]; o[2] = (float)v[2];
    }
    if (s < 3) {
        // trans.dot(R^T), then z set on the floor by frame 0 of the frame's own clip
        const double* r = a.trans_matrix + 3 * s;
        const float* t = a.src_trans + 3 * g;
        double v = (double)t[0] * r[0] + (double)t[1] * r[1] + (double)t[2] * r[2];
        if (s == 2) {
            long long lo, hi;
            clip_range(a.clip_start, a.num_clips, a.total_frames, g, lo, hi);
            const float* t0 = a.src_trans + 3 * lo;
            const double z0 = (double)t0[0] * r[0] + (double)t0[1] * r[1] + (double)t0[2] * r[2];
            v = v - (z0 - a.floor_height);
        }
        a.out_trans[3 * g + s] = (float)v;
    }
}

// launch 1: the raw quat_correct test of every (frame, body), a 32-bit word per frame
__global__ void __launch_bounds__(MsGroup::threads) motion_smooth_bits_kernel(const pulse_motion_smooth_args a) {
    const auto [slot, b, g] = lane_group<kHalfWave>();
    const int J = a.num_bodies;
    const bool frame = g < a.total_frames;
    bool flip = false;
    if (frame && b < J) {
        long long lo, hi;
        clip_range(a.clip_start, a.num_clips, a.total_frames, g, lo, hi);
        if (g > lo) {
            const Q4 p = load_q4(a.in_rot + ((g - 1) * J + b) * 4), q = load_q4(a.in_rot + (g * J + b) * 4);
            const float mx = p.x - q.x, my = p.y - q.y, mz = p.z - q.z, mw = p.w - q.w;
            const float sx = p.x + q.x, sy = p.y + q.y, sz = p.z + q.z, sw = p.w + q.w;
            flip = sqrtf(mx * mx + my * my + mz * mz + mw * mw) > sqrtf(sx * sx + sy * sy + sz * sz + sw * sw);
        }
    }
    const unsigned long long wave = __ballot(flip);        // every lane of the wave: the two frames of the wave, 32 bodies each
    const unsigned word = (threadIdx.x & kHalfWave) ? (unsigned)(wave >> 32) : (unsigned)wave;
    if (frame && b == 0) a.sign_words[g] = word;
}

// launch 2: prefix XOR of the words along every clip, in place; a wave per clip, 64 frames a step, the carry from step to step
__global__ void __launch_bounds__(kMsScanThreads) motion_smooth_scan_kernel(const pulse_motion_smooth_args a) {
    const int lane = threadIdx.x % kWave;
    const long long m = (long long)blockIdx.x * kMsScanClips + threadIdx.x / kWave;
    if (m >= a.num_clips) return;                          // whole waves leave together
    const long long total = a.total_frames;
    long long lo = a.clip_start[m], hi = a.clip_start[m + 1];
    lo = lo < 0 ? 0 : (lo > total ? total : lo);
    hi = hi < lo ? lo : (hi > total ? total : hi);
    unsigned carry = 0;
    for (long long base = lo; base < hi; base += kWave) {  // uniform over the wave
        const long long g = base + lane;
        unsigned w = g < hi ? a.sign_words[g] : 0u;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const unsigned t = __shfl_up(w, d, kWave);
            if (lane >= d) w ^= t;
        }
        w ^= carry;
        if (g < hi) a.sign_words[g] = w;
        carry = __shfl(w, kWave - 1, kWave);
    }
}

__device__ __forceinline__ Q4 signed_tap(const pulse_motion_smooth_args& a, long long g, int J, int b) {
    const Q4 q = load_q4(a.in_rot + (g * J + b) * 4);
    return ((a.sign_words[g] >> b) & 1u) ? Q4{-q.x, -q.y, -q.z, -q.w} : q;
}

// launch 3: the two Gaussian filters, the renormalisation and the local rotations
__global__ void __launch_bounds__(MsGroup::threads) motion_smooth_filter_kernel(const pulse_motion_smooth_args a, const BodyTree<kHalfWave> tree) {
    const auto [slot, b, g] = lane_group<kHalfWave>();
    const int J = a.num_bodies;
    const bool frame = g < a.total_frames;
    const bool body = frame && b < J;
    long long lo = 0, hi = 0;
    if (frame) clip_range(a.clip_start, a.num_clips, a.total_frames, g, lo, hi);
    Q4 G{0.0f, 0.0f, 0.0f, 1.0f};
    if (body) {
        const Q4 c = signed_tap(a, g, J, b);
        G = c;
        if (a.radius_rot >= 0) {
            // scipy correlate1d, symmetric filter: centre tap, then the pairs from the outermost inwards; mode "nearest" clamps to the clip
            double ax = (double)c.x * a.w_rot[0], ay = (double)c.y * a.w_rot[0], az = (double)c.z * a.w_rot[0], aw = (double)c.w * a.w_rot[0];
            for (int k = a.radius_rot; k >= 1; --k) {
                const Q4 l = signed_tap(a, g - k < lo ? lo : g - k, J, b), h = signed_tap(a, g + k > hi ? hi : g + k, J, b);
                const double w = a.w_rot[k];
                ax = ax + ((double)l.x + (double)h.x) * w;
                ay = ay + ((double)l.y + (double)h.y) * w;
                az = az + ((double)l.z + (double)h.z) * w;
                aw = aw + ((double)l.w + (double)h.w) * w;
            }
            // filtered_quats / np.linalg.norm(filtered_quats, axis=-1) on the fp32 array the filter hands back
            const Q4 f{(float)ax, (float)ay, (float)az, (float)aw};
            const float n = sqrtf(f.x * f.x + f.y * f.y + f.z * f.z + f.w * f.w);
            G = Q4{f.x / n, f.y / n, f.z / n, f.w / n};
        }
        store_q4(a.out_rot + (g * J + b) * 4, G);
    }
    // SkeletonState.local_rotation of the filtered globals (skeleton3d.py:444-460)
    const int p = b < J ? tree.parent[b] : -1;
    const Q4 Gp = lane_read(G, p < 0 ? 0 : p);
    if (body && a.out_pose_quat) store_q4(a.out_pose_quat + (g * J + b) * 4, p < 0 ? G : qmul_norm(qconj(Gp), G));
    if (frame && b < 3) {
        float v = a.in_trans[3 * g + b];
        if (a.radius_trans >= 0) {
            double acc = (double)v * a.w_trans[0];
            for (int k = a.radius_trans; k >= 1; --k) {
                const long long gl = g - k < lo ? lo : g - k, gh = g + k > hi ? hi : g + k;
                acc = acc + ((double)a.in_trans[3 * gl + b] + (double)a.in_trans[3 * gh + b]) * a.w_trans[k];
            }
            v = (float)acc;
        }
        a.out_trans[3 * g + b] = v;
    }
}

// the clip table of both entry points: host copy of the frame counts (each >= 1, sum = total_frames)
static int check_clip_frames(const char* what, const int64_t* frames, int num_clips, long long total) {
    long long sum = 0;
    for (int m = 0; m < num_clips; ++m) {
        const long long f = frames[m];
        PULSE_REQUIRE(f >= 1, "%s: clip %d has %lld frames: at least 1 is needed", what, m, f);
        PULSE_REQUIRE(f <= total - sum, "%s: the clips hold more frames than total_frames %lld (at clip %d)", what, total, m);
        sum += f;
    }
    PULSE_REQUIRE(sum == total, "%s: the clips hold %lld frames but total_frames is %lld", what, sum, total);
    return PULSE_OK;
}
static bool ranges_overlap(const void* p, long long pbytes, const void* q, long long qbytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && q && a < b + (uintptr_t)qbytes && b < a + (uintptr_t)pbytes;
}

}  // namespace pulse

extern "C" int pulse_sizeof_motion_euler_pose_args(void) { return (int)sizeof(pulse_motion_euler_pose_args); }
extern "C" int pulse_sizeof_motion_smooth_args(void) { return (int)sizeof(pulse_motion_smooth_args); }

extern "C" int pulse_motion_euler_pose(const pulse_motion_euler_pose_args* args, pulse_stream_t s) {
    using namespace pulse;
    const char* const what = "pulse_motion_euler_pose";
    PULSE_REQUIRE(args != nullptr, "%s: null args", what);
    const pulse_motion_euler_pose_args& a = *args;
    PULSE_REQUIRE(a.num_clips >= 0 && a.total_frames >= 0, "%s: negative clip / frame count", what);
    if (a.num_clips == 0 && a.total_frames == 0) return PULSE_OK;
    PULSE_REQUIRE(a.src_theta && a.src_trans, "%s: null input pointer (src_theta / src_trans)", what);
    PULSE_REQUIRE(a.clip_start && a.clip_frames_host, "%s: null clip table (clip_start / clip_frames_host)", what);
    PULSE_REQUIRE(a.out_pose && a.out_trans, "%s: null output (out_pose / out_trans)", what);
    if (const int rc = check_clip_frames(what, a.clip_frames_host, a.num_clips, a.total_frames)) return rc;
    unsigned blocks;                                       // before any byte count is formed: total_frames < 2^34 from here on
    if (const int rc = lane_group_blocks(what, a.total_frames, MsGroup::slots, blocks)) return rc;
    const long long pose_bytes = a.total_frames * 3 * kMsJoints * 4, trans_bytes = a.total_frames * 3 * 4;
    PULSE_REQUIRE(!ranges_overlap(a.src_theta, pose_bytes, a.out_pose, pose_bytes), "%s: out_pose overlaps src_theta", what);
    // a frame's z reads frame 0 of its clip: in place, another workgroup may have rewritten it
    PULSE_REQUIRE(!ranges_overlap(a.src_trans, trans_bytes, a.out_trans, trans_bytes), "%s: out_trans overlaps src_trans", what);
    hipLaunchKernelGGL(motion_euler_pose_kernel, dim3(blocks), dim3(MsGroup::threads), 0, as_stream(s), a);
    return check_launch(what);
}

extern "C" int pulse_motion_smooth(const pulse_motion_smooth_args* args, pulse_stream_t s) {
    using namespace pulse;
    const char* const what = "pulse_motion_smooth";
    static_assert(PULSE_INGEST_MAX_BODIES == kHalfWave, "one lane and one bit of a 32-bit word per body");
    PULSE_REQUIRE(args != nullptr, "%s: null args", what);
    const pulse_motion_smooth_args& a = *args;
    PULSE_REQUIRE(a.num_clips >= 0 && a.total_frames >= 0, "%s: negative clip / frame count", what);
    if (a.num_clips == 0 && a.total_frames == 0) return PULSE_OK;
    const int J = a.num_bodies;
    PULSE_REQUIRE(a.in_rot && a.in_trans, "%s: null input pointer (in_rot / in_trans)", what);
    PULSE_REQUIRE(a.clip_start && a.clip_frames_host, "%s: null clip table (clip_start / clip_frames_host)", what);
    PULSE_REQUIRE(a.sign_words, "%s: null workspace (sign_words)", what);
    PULSE_REQUIRE(a.out_rot && a.out_trans, "%s: null output (out_rot / out_trans)", what);
    BodyTree<kHalfWave> tree;
    if (const int rc = check_tree(what, a.parent_indices_host, J, tree)) return rc;
    PULSE_REQUIRE(a.radius_rot >= -1 && a.radius_rot <= kMsMaxRadius, "%s: radius_rot %d not in [-1,%d] (-1: no filter)", what, a.radius_rot, kMsMaxRadius);
    PULSE_REQUIRE(a.radius_trans >= -1 && a.radius_trans <= kMsMaxRadius, "%s: radius_trans %d not in [-1,%d] (-1: no filter)", what, a.radius_trans, kMsMaxRadius);
    if (const int rc = check_clip_frames(what, a.clip_frames_host, a.num_clips, a.total_frames)) return rc;
    unsigned blocks, scan_blocks;                          // before any byte count is formed: total_frames < 2^34 from here on
    if (const int rc = lane_group_blocks(what, a.total_frames, MsGroup::slots, blocks)) return rc;
    if (const int rc = lane_group_blocks(what, a.num_clips, kMsScanClips, scan_blocks)) return rc;
    PULSE_REQUIRE(reinterpret_cast<uintptr_t>(a.in_rot) % 16 == 0, "%s: in_rot must be 16-byte aligned", what);
    PULSE_REQUIRE(reinterpret_cast<uintptr_t>(a.out_rot) % 16 == 0, "%s: out_rot must be 16-byte aligned", what);
    PULSE_REQUIRE(reinterpret_cast<uintptr_t>(a.out_pose_quat) % 16 == 0, "%s: out_pose_quat must be 16-byte aligned", what);
    const long long rot_bytes = a.total_frames * J * 16, trans_bytes = a.total_frames * 12;
    PULSE_REQUIRE(!ranges_overlap(a.in_rot, rot_bytes, a.out_rot, rot_bytes), "%s: out_rot overlaps in_rot: the filter reads its neighbours' unfiltered values", what);
    PULSE_REQUIRE(!ranges_overlap(a.in_rot, rot_bytes, a.out_pose_quat, rot_bytes), "%s: out_pose_quat overlaps in_rot: the filter reads its neighbours' unfiltered values", what);
    PULSE_REQUIRE(!ranges_overlap(a.out_rot, rot_bytes, a.out_pose_quat, rot_bytes), "%s: out_pose_quat overlaps out_rot", what);
    PULSE_REQUIRE(!ranges_overlap(a.in_trans, trans_bytes, a.out_trans, trans_bytes), "%s: out_trans overlaps in_trans: the filter reads its neighbours' unfiltered values", what);
    const void* const buf[5] = {a.in_rot, a.out_rot, a.out_pose_quat, a.in_trans, a.out_trans};
    for (int i = 0; i < 5; ++i)
        PULSE_REQUIRE(!ranges_overlap(a.sign_words, a.total_frames * 4, buf[i], i < 3 ? rot_bytes : trans_bytes), "%s: sign_words overlaps a data buffer", what);
    hipLaunchKernelGGL(motion_smooth_bits_kernel, dim3(blocks), dim3(MsGroup::threads), 0, as_stream(s), a);
    hipLaunchKernelGGL(motion_smooth_scan_kernel, dim3(scan_blocks), dim3(kMsScanThreads), 0, as_stream(s), a);
    hipLaunchKernelGGL(motion_smooth_filter_kernel, dim3(blocks), dim3(MsGroup::threads), 0, as_stream(s), a, tree);
    return check_launch(what);
}
