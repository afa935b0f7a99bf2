// A streamed keypoint reference (include/pulse_hip.h section 2b'.3), on gfx950: the host work HumanoidImMCPDemo._compute_task_obs_demo does every
// control step in front of the task observation (phc/env/tasks/humanoid_im_mcp_demo.py:252-290) -- reorder, root-relative, limb-length scale,
// append to the history, the newest sample of three mirror-mode Gaussian filters, frame change, finite-difference velocity -- for every env in
// one launch per pushed frame.
//
// A 32-lane half-wave per env, eight envs per 256-thread workgroup.  Nothing goes through LDS and there is no barrier:
//   lane b < J  <-> BODY b: its keypoint (three dwords), its share of the limb scale, its three ring coordinates, its pos / vel / prev_pos rows;
//   lane J      <-> the ROOT translation: the same three-coordinate tap sum over the root ring, with the root's two tap tables; the body lanes
//                   fetch its result with three cross-lane reads.
// The other mapping, lane = coordinate (72 + 3 per env), splits an env over two waves: the 3 x 3 frame product and the root sum would cross them
// through LDS and a barrier, for a launch whose cost is its latency (8 workgroups at 64 envs).  With lane = body the three coordinates of a body
// stay in one lane and 25 of 32 lanes work.  The rings are slot-major inside the env ((N, H, J, 3)): the body lanes of an env read ONE contiguous
// run of 12 J bytes per slot (288 at J = 24), three dwords per lane, and the L slots of an env are L such runs; the tap of a slot is one address
// for every body lane of the env.
// The two envs of a wave may hold different L: the tap loop runs to each lane's own L - 1 (the wave iterates to the longer one).  No lane returns
// early: every lane of the wave executes every cross-lane read.
// Memory bound, latency bound at small N.  Per env and push at J = 24, L = H = 30: read 288 (keypoints) + 29 x 300 (rings) + 288 (prev_pos)
// + 4 (count) + taps (cached: 3 x 30 floats), written 300 (ring slot) + 3 x 288 (pos, vel, prev_pos) + 288 (raw) + 4.
// Measured: profiles/keypoint_stream.txt.
// Compiled with -ffp-contract=off: fp32 in the operation order of the numpy statements.
#include "body_lanes.h"
#include "env_select.h"

namespace pulse {

using KpGroup = LaneGroup<kHalfWave>;            // lanes per env: J bodies + the root lane

// what the launcher validated on the host, by value in the kernel arguments
struct KpTables {
    unsigned char joint[kHalfWave];               // body -> SMPL joint
    unsigned char limb_parent[PULSE_KEYPOINT_LIMBS];
};

__global__ void __launch_bounds__(KpGroup::threads) keypoint_push_kernel(const pulse_keypoint_push_args a, const KpTables tb) {
    const auto [slot, b, e] = lane_group<kHalfWave>();
    const int J = a.num_bodies, H = a.history;
    const bool env = env_enabled(a, e);                                           // no early return: every lane reaches every cross-lane read
    const bool body = env && b < J, root = env && b == J;
    const bool lane = body || root;

    // ---- the keypoint of the lane (the root lane takes body 0's: trans), reordered; raw goes out as it came in
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (lane) {
        const float* k = a.j3d + e * a.j3d_stride_n + (long long)tb.joint[body ? b : 0] * a.j3d_stride_j;
        px = k[0]; py = k[1]; pz = k[2];
    }
    if (body && a.raw) { float* o = a.raw + (e * J + b) * 3; o[0] = px; o[1] = py; o[2] = pz; }
    const float tx = __shfl(px, J, kHalfWave), ty = __shfl(py, J, kHalfWave), tz = __shfl(pz, J, kHalfWave);      // trans = p[0]
    float qx = px - tx, qy = py - ty, qz = pz - tz;                                // p -= trans
    // ---- limb-length scale: lanes 1 .. 5 take |p[parent] - p[own]| / mean length; every lane sums the five in order
    const int par = (b >= 1 && b <= PULSE_KEYPOINT_LIMBS) ? tb.limb_parent[b - 1] : 0;
    const float dx = __shfl(qx, par, kHalfWave) - qx, dy = __shfl(qy, par, kHalfWave) - qy, dz = __shfl(qz, par, kHalfWave) - qz;
    const float ratio = sqrtf(dx * dx + dy * dy + dz * dz) / a.mean_limb_lengths[(b >= 1 && b <= PULSE_KEYPOINT_LIMBS) ? b - 1 : 0];
    float scale = __shfl(ratio, 1, kHalfWave);
#pragma unroll
    for (int i = 2; i <= PULSE_KEYPOINT_LIMBS; ++i) scale = scale + __shfl(ratio, i, kHalfWave);
    scale = scale / (float)PULSE_KEYPOINT_LIMBS;
    if (root) { qx = tx; qy = ty; qz = tz; }                                       // the root lane carries trans itself, unscaled
    else { qx = qx / scale; qy = qy / scale; qz = qz / scale; }                    // scale 0: 0 / 0 = NaN, as numpy

    // ---- append: slot w of the env's ring; L samples are valid afterwards
    int c = 0;
    if (lane) { c = a.count[e]; c = c < 0 ? 0 : c; }
    const int w = c % H, L = (c + 1 < H) ? c + 1 : H;
    // the lane's ring: (H, stride) floats from ``ring``, its three coordinates at ``at``
    float* ring = nullptr;
    int stride = 0;
    if (body) { ring = a.body_ring + e * H * J * 3 + b * 3; stride = J * 3; }
    if (root) { ring = a.root_ring + e * H * 3; stride = 3; }
    if (lane) { float* o = ring + w * stride; o[0] = qx; o[1] = qy; o[2] = qz; }
    // ---- the newest sample of the mirror-mode Gaussian: row L - 1 of the lane's tap tables, oldest sample first
    const float* t01 = a.taps + ((long long)(root ? 1 : 2) * H + (L - 1)) * H;     // coordinates 0, 1: sigma 5 for the root, sigma 2 for a body
    const float* t2 = a.taps + ((long long)(root ? 0 : 2) * H + (L - 1)) * H;      // coordinate 2: sigma 10 for the root
    float fx = 0.0f, fy = 0.0f, fz = 0.0f;
    if (lane) {
        int s = w - (L - 1);                                                        // the oldest valid slot
        s = s < 0 ? s + H : s;
        for (int i = 0; i < L - 1; ++i) {
            const float* r = ring + s * stride;
            const float w01 = t01[i], w2 = t2[i];
            fx = fx + w01 * r[0]; fy = fy + w01 * r[1]; fz = fz + w2 * r[2];
            s = s + 1 == H ? 0 : s + 1;
        }
        const float w01 = t01[L - 1], w2 = t2[L - 1];                              // the sample just appended, from its registers
        fx = fx + w01 * qx; fy = fy + w01 * qy; fz = fz + w2 * qz;
    }
    // ---- pos = frame (p_f + trans_f); vel = (pos - prev_pos) / dt
    const float x0 = fx + __shfl(fx, J, kHalfWave), x1 = fy + __shfl(fy, J, kHalfWave), x2 = fz + __shfl(fz, J, kHalfWave);
    if (body) {
        const long long at = (e * J + b) * 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float p = a.frame[3 * i] * x0 + a.frame[3 * i + 1] * x1 + a.frame[3 * i + 2] * x2;
            const float v = (p - a.prev_pos[at + i]) / a.dt;
            a.pos[at + i] = p;
            a.vel[at + i] = v;
            a.prev_pos[at + i] = p;
        }
    }
    if (root) {
        int next = c + 1;
        if (next >= (1 << 30)) next = H + next % H;                                // keeps L = H and the slot
        a.count[e] = next;
    }
}

}  // namespace pulse

extern "C" int pulse_sizeof_keypoint_push_args(void) { return (int)sizeof(pulse_keypoint_push_args); }

extern "C" int pulse_keypoint_push(const pulse_keypoint_push_args* args, pulse_stream_t s) {
    using namespace pulse;
    static_assert(PULSE_KEYPOINT_MAX_BODIES == kHalfWave - 1, "one lane per body and one for the root");
    PULSE_REQUIRE(args != nullptr, "pulse_keypoint_push: null args");
    const pulse_keypoint_push_args& a = *args;
    PULSE_REQUIRE(a.num_envs >= 0, "pulse_keypoint_push: negative num_envs");
    if (a.num_envs == 0) return PULSE_OK;
    const int J = a.num_bodies, H = a.history;
    PULSE_REQUIRE(J > PULSE_KEYPOINT_LIMBS && J <= PULSE_KEYPOINT_MAX_BODIES,
                  "pulse_keypoint_push: num_bodies %d not in [6,31] (bodies 1 .. 5 are the limbs; one lane of a half-wave per body and one for the root)", J);
    PULSE_REQUIRE(H >= 1 && H <= PULSE_KEYPOINT_MAX_HISTORY, "pulse_keypoint_push: history %d not in [1,64]", H);
    PULSE_REQUIRE(a.dt > 0.0f, "pulse_keypoint_push: dt %g must be positive", (double)a.dt);
    PULSE_REQUIRE(a.j3d != nullptr, "pulse_keypoint_push: null j3d");
    PULSE_REQUIRE(a.j3d_stride_n >= 0 && a.j3d_stride_j >= 3, "pulse_keypoint_push: j3d strides (%lld, %lld): non-negative, and at least 3 floats between joints",
                  (long long)a.j3d_stride_n, (long long)a.j3d_stride_j);
    PULSE_REQUIRE(a.taps != nullptr, "pulse_keypoint_push: null taps");
    PULSE_REQUIRE(a.root_ring && a.body_ring && a.count && a.prev_pos, "pulse_keypoint_push: null state (root_ring / body_ring / count / prev_pos)");
    PULSE_REQUIRE(a.pos && a.vel, "pulse_keypoint_push: null output (pos / vel)");
    KpTables tb = {};
    if (const int rc = check_permutation<kHalfWave>("pulse_keypoint_push", "joint_map", a.joint_map, J, nullptr)) return rc;
    for (int b = 0; b < J; ++b) tb.joint[b] = (unsigned char)a.joint_map[b];
    BodyTree<kHalfWave> tree;
    if (const int rc = check_tree("pulse_keypoint_push", a.parent_indices, J, tree)) return rc;
    for (int i = 0; i < PULSE_KEYPOINT_LIMBS; ++i) tb.limb_parent[i] = (unsigned char)tree.parent[i + 1];
    unsigned blocks;
    if (const int rc = lane_group_blocks("pulse_keypoint_push", a.num_envs, KpGroup::slots, blocks)) return rc;
    hipLaunchKernelGGL(keypoint_push_kernel, dim3(blocks), dim3(KpGroup::threads), 0, as_stream(s), a, tb);
    return check_launch("pulse_keypoint_push");
}
