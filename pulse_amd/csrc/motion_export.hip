// A recorded rollout -> motion clips and SMPL pose sequences (include/pulse_hip.h section 2b'.2), on gfx950: the mirror image of
// motion_ingest.hip.  What HumanoidIm.render (phc/env/tasks/humanoid_im.py:217-257) and Humanoid._write_states_to_file
// (phc/env/tasks/humanoid.py:439-491) compute frame by frame with scipy, poselib and torch on the CPU -- here one launch over every output
// frame of every segment of the recording, read in place.
//
// A 32-lane half-wave per output frame, eight frames per 256-thread workgroup.  Nothing goes through LDS and there is no barrier:
//   lane b <-> BODY b: loads its global rotation from the recording (four dwords of its 13-float row) and stores it unchanged; the upright
//     factor scipy-style; the local rotation from ONE read of the parent's lane; scipy's as_rotvec of it; the dump's body_quat from its own
//     three dof_pos floats.  Each lane stores its own float4, so a frame's (J, 4) row is one contiguous run of 16-byte stores;
//   lane s <-> SMPL joint s: fetches the rotation vector of the body b with joint_map[b] == s from that lane and writes pose_aa (a coalesced row).
// The lanes of a half-wave whose frame lies past the end, and lanes >= J, run along with identity rotations and store nothing: every
// lane of the wave executes every cross-lane read.
// Memory bound.  The rb rows are 52 bytes apart and only 16 of them (28 for the root) are used: a frame's J rows are one contiguous run of
// 52 J bytes, every 128-byte line of which is fetched -- at J = 24 a run of 1248 bytes lies in ten lines, eleven when it straddles: 1280 or
// 1408 bytes fetched for the 396 used, 3.2 - 3.6 x; a float4 load is not possible at that pitch.  Written per frame: 16 J + 12 (396 at J = 24), and
// with the optional outputs 16 J + 12 J + 12 (pose_quat, pose_aa, trans_orig: 684) + 16 J + 12 (J - 1) (body_quat, dof_pos: 660) more, 1740 in all.
// Measured: profiles/motion_export.txt.
// Compiled with -ffp-contract=off: fp32 in the operation order of scipy / poselib / torch_utils.
#include "poselib_math.h"

namespace pulse {

using MxGroup = LaneGroup<kHalfWave>;            // lanes per frame = PULSE_EXPORT_MAX_BODIES

// the parents of the tree (the kernel reads no depth) and the inverse joint map, by value in the kernel arguments (from the launcher's validated host copies)
struct MxTree { signed char parent[kHalfWave]; unsigned char body_of_joint[kHalfWave]; };

__global__ void __launch_bounds__(MxGroup::threads) motion_export_kernel(const pulse_motion_export_args a, const MxTree tree) {
    const auto [slot, b, g] = lane_group<kHalfWave>();
    const int J = a.num_bodies;
    const bool frame = g < a.total_frames;                 // no early return: every lane reaches every cross-lane read
    const bool body = frame && b < J;
    long long t = 0, env = 0;
    if (frame) {
        const int m = clip_of(a.seg_out_start, a.num_segments, g);
        t = a.seg_t0[m] + (g - a.seg_out_start[m]);
        env = a.seg_env[m];
        t = t < 0 ? 0 : (t > a.num_steps - 1 ? a.num_steps - 1 : t);                     // a bad segment table reads a wrong frame, never out of bounds
        env = env < 0 ? 0 : (env > a.num_envs - 1 ? a.num_envs - 1 : env);
    }
    const float* row = a.rb + t * a.rb_stride_t + env * a.rb_stride_n;
    Q4 G{0.0f, 0.0f, 0.0f, 1.0f};
    if (body) {
        const float* r = row + b * a.rb_stride_b + 3;
        G = Q4{r[0], r[1], r[2], r[3]};
        store_q4(a.out_rot + (g * J + b) * 4, G);
    }
    if (frame && b < 3) {
        const float p = row[b];
        a.out_trans[3 * g + b] = p;
        if (a.out_trans_orig) a.out_trans_orig[3 * g + b] = p - a.root_offset[b];
    }
    // the joint's exponential map (dof_pos), body b >= 1
    V3 e{0.0f, 0.0f, 0.0f};
    const bool has_dof = a.dof_pos != nullptr;
    if (body && b >= 1 && has_dof) {
        const float* d = a.dof_pos + t * a.dof_stride_t + env * a.dof_stride_n + 3 * (b - 1);
        e = V3{d[0], d[1], d[2]};
        if (a.out_dof_pos) { float* o = a.out_dof_pos + g * (3 * (J - 1)) + 3 * (b - 1); o[0] = e.x; o[1] = e.y; o[2] = e.z; }
    }
    // the dump's body_quat = [root quat, exp_map_to_quat(dof_pos)]
    const Q4 bq = b == 0 ? G : exp_map_to_q(e);
    if (body && a.out_body_quat) store_q4(a.out_body_quat + (g * J + b) * 4, bq);
    Q4 l;
    V3 rv;
    if (a.upright_start) {                                 // uniform over the launch
        const int p = b < J ? tree.parent[b] : -1;
        // (sRot.from_quat(g) * sRot.from_quat([0.5, 0.5, 0.5, 0.5])).as_quat(): normalise, compose, normalise
        const Q4 Gu = qunit_scipy(qcompose_scipy(qunit_scipy(G), Q4{0.5f, 0.5f, 0.5f, 0.5f}));
        // SkeletonState.local_rotation of those globals (skeleton3d.py:444-460): one parent read per lane
        const Q4 Gp = lane_read(Gu, p < 0 ? 0 : p);
        l = p < 0 ? Gu : qmul_norm(qconj(Gp), Gu);
        rv = quat_to_rotvec_scipy(l);
    } else {
        l = bq;
        rv = b == 0 ? q_to_exp_map(G) : e;
    }
    if (body && a.out_pose_quat) store_q4(a.out_pose_quat + (g * J + b) * 4, l);
    // lane <-> SMPL joint: pose_aa[:, mujoco_2_smpl]
    const V3 aa = lane_read(rv, b < J ? tree.body_of_joint[b] : 0);
    if (body && a.out_pose_aa) { float* o = a.out_pose_aa + g * (3 * J) + 3 * b; o[0] = aa.x; o[1] = aa.y; o[2] = aa.z; }
}

}  // namespace pulse

extern "C" int pulse_sizeof_motion_export_args(void) { return (int)sizeof(pulse_motion_export_args); }

extern "C" int pulse_motion_export(const pulse_motion_export_args* args, pulse_stream_t s) {
    using namespace pulse;
    static_assert(PULSE_EXPORT_MAX_BODIES == kHalfWave, "one lane per body");
    PULSE_REQUIRE(args != nullptr, "pulse_motion_export: null args");
    const pulse_motion_export_args& a = *args;
    PULSE_REQUIRE(a.num_segments >= 0 && a.total_frames >= 0, "pulse_motion_export: negative segment / frame count");
    if (a.num_segments == 0 && a.total_frames == 0) return PULSE_OK;
    const int J = a.num_bodies;
    PULSE_REQUIRE(J >= 1 && J <= kHalfWave, "pulse_motion_export: num_bodies %d not in [1,32] (one lane of a half-wave per body)", J);
    PULSE_REQUIRE(a.rb != nullptr, "pulse_motion_export: null recording (rb)");
    PULSE_REQUIRE(a.num_steps >= 1 && a.num_envs >= 1, "pulse_motion_export: the recording is empty (num_steps %lld, num_envs %d)", (long long)a.num_steps, a.num_envs);
    PULSE_REQUIRE(a.rb_stride_t >= 0 && a.rb_stride_n >= 0 && a.rb_stride_b >= 13,
                  "pulse_motion_export: rb strides (%lld, %lld, %lld): non-negative, and at least 13 floats between bodies",
                  (long long)a.rb_stride_t, (long long)a.rb_stride_n, (long long)a.rb_stride_b);
    PULSE_REQUIRE(a.dof_pos == nullptr || (a.dof_stride_t >= 0 && a.dof_stride_n >= 0), "pulse_motion_export: negative dof_pos stride");
    PULSE_REQUIRE(a.seg_env && a.seg_t0 && a.seg_out_start, "pulse_motion_export: null per-segment table (seg_env / seg_t0 / seg_out_start)");
    PULSE_REQUIRE(a.seg_env_host && a.seg_t0_host && a.seg_frames_host,
                  "pulse_motion_export: null host table (seg_env_host / seg_t0_host / seg_frames_host)");
    PULSE_REQUIRE(a.out_rot && a.out_trans, "pulse_motion_export: null output (out_rot / out_trans)");
    PULSE_REQUIRE(a.dof_pos != nullptr || !(a.out_body_quat || a.out_dof_pos), "pulse_motion_export: out_body_quat / out_dof_pos need dof_pos");
    PULSE_REQUIRE(a.dof_pos != nullptr || a.upright_start || !(a.out_pose_quat || a.out_pose_aa),
                  "pulse_motion_export: without upright_start out_pose_quat / out_pose_aa need dof_pos");
    BodyTree<kHalfWave> checked;
    if (const int rc = check_tree("pulse_motion_export", a.parent_indices_host, J, checked)) return rc;
    MxTree tree = {};
    for (int b = 0; b < kHalfWave; ++b) tree.parent[b] = checked.parent[b];
    if (const int rc = check_permutation<kHalfWave>("pulse_motion_export", "joint_map", a.joint_map, J, tree.body_of_joint)) return rc;
    long long sum = 0;
    for (int m = 0; m < a.num_segments; ++m) {
        const long long f = a.seg_frames_host[m], t0 = a.seg_t0_host[m], e = a.seg_env_host[m];
        PULSE_REQUIRE(f >= 1, "pulse_motion_export: segment %d has %lld frames: at least 1 is needed", m, f);
        PULSE_REQUIRE(e >= 0 && e < a.num_envs, "pulse_motion_export: segment %d is of env %lld, outside [0,%d)", m, e, a.num_envs);
        // t0 + f is not formed before it is known to fit
        PULSE_REQUIRE(t0 >= 0 && t0 < a.num_steps && f <= a.num_steps - t0,
                      "pulse_motion_export: segment %d reads %lld steps from %lld, outside [0,%lld)", m, f, t0, (long long)a.num_steps);
        PULSE_REQUIRE(f <= 0x7fffffffLL * MxGroup::slots - sum, "pulse_motion_export: %lld and more frames exceed the grid", sum + f);
        sum += f;
    }
    PULSE_REQUIRE(sum == a.total_frames, "pulse_motion_export: the segments hold %lld frames but total_frames is %lld", sum, (long long)a.total_frames);
    PULSE_REQUIRE(reinterpret_cast<uintptr_t>(a.out_rot) % 16 == 0, "pulse_motion_export: out_rot must be 16-byte aligned");
    PULSE_REQUIRE(reinterpret_cast<uintptr_t>(a.out_pose_quat) % 16 == 0, "pulse_motion_export: out_pose_quat must be 16-byte aligned");
    PULSE_REQUIRE(reinterpret_cast<uintptr_t>(a.out_body_quat) % 16 == 0, "pulse_motion_export: out_body_quat must be 16-byte aligned");
    unsigned blocks;
    if (const int rc = lane_group_blocks("pulse_motion_export", a.total_frames, MxGroup::slots, blocks)) return rc;
    hipLaunchKernelGGL(motion_export_kernel, dim3(blocks), dim3(MxGroup::threads), 0, as_stream(s), a, tree);
    return check_launch("pulse_motion_export");
}
