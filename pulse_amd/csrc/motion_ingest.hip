// Raw SMPL pose sequences -> the converted motion data MotionLib stages (include/pulse_hip.h section 2b'.1), on gfx950: what
// scripts/data_process/convert_amass_isaac.py:85-137 and convert_amass_data.py:88-141 compute clip by clip with scipy and poselib on the
// CPU -- here one launch over every output frame of every clip.
//
// A 32-lane half-wave per output frame, eight frames per 256-thread workgroup.  Nothing goes through LDS and there is no barrier:
//   lane s <-> SMPL joint s (24 of the 32 lanes): loads its three axis-angle floats (a coalesced row read), zeroes the hand columns, writes pose_aa;
//   lane b <-> BODY b: fetches the axis-angle of SMPL joint joint_map[b] from that lane (ds_bpermute), scipy's from_rotvec in fp32,
//     then the forward pass down the tree one level per round, each lane reading its parent's global rotation from the parent's lane;
//     the upright factor; the local rotations back from the new globals (one more parent read); the mirrored copy reads lane
//     mirror_map[b].  Each lane stores its own float4, so a frame's (J, 4) row is one contiguous run of 16-byte stores.
// The lanes of a half-wave whose frame lies past the end, and lanes >= J, run along with identity rotations and store nothing: every
// lane of the wave executes every cross-lane read.  Memory bound: 300 bytes read and 16 J + 12 (+ 16 J + 300 with the optional
// outputs) written per frame.  Measured: profiles/motion_ingest.txt.
// Compiled with -ffp-contract=off: fp32 in the operation order of scipy / poselib.
#include "poselib_math.h"

namespace pulse {

using MiGroup = LaneGroup<kHalfWave>;            // lanes per frame = PULSE_INGEST_MAX_BODIES
constexpr int kMiJoints = PULSE_INGEST_SMPL_JOINTS, kMiHandCol = PULSE_INGEST_SMPL_HAND_COL;

__global__ void __launch_bounds__(MiGroup::threads) motion_ingest_kernel(const pulse_motion_ingest_args a, const BodyTree<kHalfWave> tree) {
    const auto [slot, b, g] = lane_group<kHalfWave>();
    const int J = a.num_bodies;
    const bool frame = g < a.total_frames;                 // no early return: every lane reaches every cross-lane read
    const bool body = frame && b < J;
    long long src = 0;
    int mirror = 0;
    if (frame) {
        const int m = clip_of(a.clip_out_start, a.num_clips, g);
        src = a.clip_src_start[m] + (g - a.clip_out_start[m]) * a.clip_skip[m];
        src = src < 0 ? 0 : (src > a.src_frames - 1 ? a.src_frames - 1 : src);          // a bad clip table reads a wrong frame, never out of bounds
        mirror = a.clip_mirror ? (int)a.clip_mirror[m] : 0;
    }
    // lane <-> SMPL joint: pose_aa = [poses[:, :66], 0]
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    if (frame && b < kMiJoints) {
        if (3 * b < kMiHandCol) {
            const float* p = a.src_pose + src * (3 * kMiJoints) + 3 * b;
            ax = p[0]; ay = p[1]; az = p[2];
        }
        if (a.out_pose_aa) { float* o = a.out_pose_aa + g * (3 * kMiJoints) + 3 * b; o[0] = ax; o[1] = ay; o[2] = az; }
    }
    // lane <-> body: pose_aa.reshape(-1, 24, 3)[:, smpl_2_mujoco] -> from_rotvec
    const int jm = b < J ? a.joint_map[b] : 0;
    const V3 aa = lane_read(V3{ax, ay, az}, jm);
    const Q4 q = rotvec_to_quat(aa.x, aa.y, aa.z);
    // SkeletonState.global_rotation of local rotations: transform_mul's quat_mul_norm down the tree, the root as scipy gave it
    const int p = b < J ? tree.parent[b] : -1, ps = p < 0 ? 0 : p;
    const int depth = b < J ? tree.depth[b] : 0;
    Q4 G = q;
    for (int lvl = 1; lvl <= tree.max_depth; ++lvl) {
        const Q4 Gp = lane_read(G, ps);
        if (depth == lvl) G = qmul_norm(Gp, q);
    }
    Q4 l = q;
    if (a.upright_start) {
        // (sRot.from_quat(g) * sRot.from_quat([0.5, 0.5, 0.5, 0.5]).inv()).as_quat(): normalise, compose, normalise
        G = qunit_scipy(qcompose_scipy(qunit_scipy(G), Q4{-0.5f, -0.5f, -0.5f, 0.5f}));
        // SkeletonState.local_rotation of the new globals (skeleton3d.py:444-460)
        const Q4 Gp = lane_read(G, ps);
        l = p < 0 ? G : qmul_norm(qconj(Gp), G);
    }
    if (body && a.out_pose_quat) store_q4(a.out_pose_quat + (g * J + b) * 4, l);
    // the mirrored copy: pose_quat_global[:, left_to_right_index], x and z negated
    const Q4 Gm = lane_read(G, b < J ? a.mirror_map[b] : 0);
    if (mirror) G = Q4{-Gm.x, Gm.y, -Gm.z, Gm.w};
    if (body) store_q4(a.out_rot + (g * J + b) * 4, G);
    if (frame && b < 3) {
        const float t = a.src_trans[3 * src + b];
        const float o = t + a.root_offset[b];
        a.out_trans[3 * g + b] = (mirror && b == 1) ? -o : o;
        if (a.out_trans_orig) a.out_trans_orig[3 * g + b] = t;
    }
}

}  // namespace pulse

extern "C" int pulse_sizeof_motion_ingest_args(void) { return (int)sizeof(pulse_motion_ingest_args); }

extern "C" int pulse_motion_ingest(const pulse_motion_ingest_args* args, pulse_stream_t s) {
    using namespace pulse;
    static_assert(PULSE_INGEST_MAX_BODIES == kHalfWave, "one lane per body");
    PULSE_REQUIRE(args != nullptr, "pulse_motion_ingest: null args");
    const pulse_motion_ingest_args& a = *args;
    PULSE_REQUIRE(a.num_clips >= 0 && a.total_frames >= 0, "pulse_motion_ingest: negative clip / frame count");
    if (a.num_clips == 0 && a.total_frames == 0) return PULSE_OK;
    const int J = a.num_bodies;
    static_assert(kMiJoints <= kHalfWave && kMiHandCol % 3 == 0, "one lane per SMPL joint; the hand columns start at a joint");
    PULSE_REQUIRE(J >= 1 && J <= kHalfWave, "pulse_motion_ingest: num_bodies %d not in [1,32] (one lane of a half-wave per body)", J);
    PULSE_REQUIRE(a.src_pose && a.src_trans, "pulse_motion_ingest: null staging pointer (src_pose / src_trans)");
    PULSE_REQUIRE(a.src_frames >= 1, "pulse_motion_ingest: src_frames %lld: the staging buffers are empty", (long long)a.src_frames);
    PULSE_REQUIRE(a.clip_src_start && a.clip_skip && a.clip_out_start, "pulse_motion_ingest: null per-clip table (clip_src_start / clip_skip / clip_out_start)");
    PULSE_REQUIRE(a.clip_src_start_host && a.clip_skip_host && a.clip_frames_host,
                  "pulse_motion_ingest: null host table (clip_src_start_host / clip_skip_host / clip_frames_host)");
    PULSE_REQUIRE(a.out_rot && a.out_trans, "pulse_motion_ingest: null output (out_rot / out_trans)");
    BodyTree<kHalfWave> tree;
    if (const int rc = check_tree("pulse_motion_ingest", a.parent_indices_host, J, tree)) return rc;
    for (int b = 0; b < J; ++b) {
        PULSE_REQUIRE(a.joint_map[b] >= 0 && a.joint_map[b] < kMiJoints, "pulse_motion_ingest: joint_map[%d] = %d is no SMPL joint (0 .. %d)", b, a.joint_map[b], kMiJoints - 1);
        PULSE_REQUIRE(a.mirror_map[b] >= 0 && a.mirror_map[b] < J, "pulse_motion_ingest: mirror_map[%d] = %d is no body (0 .. %d)", b, a.mirror_map[b], J - 1);
    }
    long long sum = 0;
    for (int m = 0; m < a.num_clips; ++m) {
        const long long f = a.clip_frames_host[m], k = a.clip_skip_host[m], s0 = a.clip_src_start_host[m];
        PULSE_REQUIRE(f >= 1, "pulse_motion_ingest: clip %d has %lld frames: at least 1 is needed", m, f);
        PULSE_REQUIRE(k >= 1, "pulse_motion_ingest: clip %d has skip %lld: the decimation step int(framerate / 30) must be >= 1", m, k);
        // (f - 1) * k is not formed before it is known to fit: the last frame read is s0 + (f - 1) * k <= src_frames - 1
        PULSE_REQUIRE(s0 >= 0 && s0 < a.src_frames && f - 1 <= (a.src_frames - 1 - s0) / k,
                      "pulse_motion_ingest: clip %d reads %lld staged frames from %lld in steps of %lld, outside [0,%lld)", m, f, s0, k, (long long)a.src_frames);
        sum += f;
    }
    PULSE_REQUIRE(sum == a.total_frames, "pulse_motion_ingest: the clips hold %lld frames but total_frames is %lld", sum, (long long)a.total_frames);
    PULSE_REQUIRE(reinterpret_cast<uintptr_t>(a.out_rot) % 16 == 0, "pulse_motion_ingest: out_rot must be 16-byte aligned");
    PULSE_REQUIRE(reinterpret_cast<uintptr_t>(a.out_pose_quat) % 16 == 0, "pulse_motion_ingest: out_pose_quat must be 16-byte aligned");
    unsigned blocks;
    if (const int rc = lane_group_blocks("pulse_motion_ingest", a.total_frames, MiGroup::slots, blocks)) return rc;
    hipLaunchKernelGGL(motion_ingest_kernel, dim3(blocks), dim3(MiGroup::threads), 0, as_stream(s), a, tree);
    return check_launch("pulse_motion_ingest");
}
