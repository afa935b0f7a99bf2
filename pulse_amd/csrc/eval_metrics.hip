// pulse_im_eval_accum (include/pulse_hip.h section 2b''): per-control-step accumulation of the evaluation metrics of IMAmpAgent.eval
// (phc/learning/im_amp.py:270-292, 314-341; phc/env/tasks/humanoid_im.py:667-673).  The reference copies every env's body positions to
// the host on every step and computes smpl_sim's compute_metrics_lite in numpy once the sweep is over; here the five per-frame terms are
// summed per env on the device, in fp64, and only the (N, 8) accumulator rows are read back, once per batch.
//
// Same idiom as env_step.hip: one lane group per env, lane = body; LB = 32 lanes up to 32 bodies (4 envs per workgroup), LB = 64 for
// 33 .. 64 (2 envs per workgroup).  Every per-env reduction is a butterfly shuffle (lane_sum, common.h), so all lanes of a group hold every sum (the 3 x 3 SVD
// runs redundantly on all of them) and lanes J .. LB - 1 feed exact zeros.  No atomics, no LDS.
#include <cstdint>
#include "body_lanes.h"
#include "env_select.h"

namespace pulse {
namespace {

constexpr int kEvalThreads = 128;

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// One-sided (Hestenes) Jacobi on the columns of the 3 x 3 matrix A: A V = U Sigma, V a product of plane rotations (det + 1).  Columns
// are rotated in place until mutually orthogonal; a fixed number of sweeps.  Convergence is quadratic: in an fp64 port of this loop every
// H of tests/eval_metrics_cases.py, rank-deficient ones included, stopped moving by more than 1e-15 after 2 - 4 sweeps (one took 8).  The
// skip test below asks for more than rounding leaves of a full-rank H, so the later sweeps go on turning by angles of about 1e-17, which
// moves nothing.  Afterwards sigma_i = |A[:, i]| and U[:, i] = A[:, i] / sigma_i, in no particular order; the column of a zero singular
// value ends as zero or as a remnant far below kRankTol, wherever the squares underflowed.
constexpr int kJacobiSweeps = 12;
// A column of U Sigma this much shorter than the longest is not normalised but completed (im_eval_accum_kernel).  The sums of up to 64 products
// that build H (|H| <= 1) carry about 8 eps = 2e-15 of rounding, which is the size a zero singular value comes out at; 1e-13 is well above
// that, and a true singular value below it changes the trace, and so the scale, by less than 1e-13 of itself.
constexpr double kRankTol = 1e-13;
__device__ __forceinline__ void jacobi_svd3(double A[3][3], double V[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) V[i][k] = (i == k) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
#pragma unroll
        for (int pair = 0; pair < 3; ++pair) {
            const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2;
            const double alpha = A[0][p] * A[0][p] + A[1][p] * A[1][p] + A[2][p] * A[2][p];
            const double beta = A[0][q] * A[0][q] + A[1][q] * A[1][q] + A[2][q] * A[2][q];
            const double gamma = A[0][p] * A[0][q] + A[1][p] * A[1][q] + A[2][p] * A[2][q];
            if (gamma == 0.0 || gamma * gamma <= 1e-34 * alpha * beta) continue;      // already orthogonal to ~1e-17 of their lengths
            const double zeta = (beta - alpha) / (2.0 * gamma);
            const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double ap = A[r][p], aq = A[r][q];
                A[r][p] = c * ap - s * aq;
                A[r][q] = s * ap + c * aq;
                const double vp = V[r][p], vq = V[r][q];
                V[r][p] = c * vp - s * vq;
                V[r][q] = s * vp + c * vq;
            }
        }
    }
}

template <int LB>
__global__ void __launch_bounds__(kEvalThreads) im_eval_accum_kernel(const pulse_im_eval_args a) {
    constexpr int E = kEvalThreads / LB;
    const int J = a.num_bodies;
    const int lane = threadIdx.x % LB;
    const int e = blockIdx.x * E + threadIdx.x / LB;
    if (!env_enabled(a, e)) return;                           // whole groups leave together: the shuffles below stay inside a group
    const int s = a.step;
    const bool body = lane < J;

    // this step's positions, widened once
    double P[3] = {0.0, 0.0, 0.0}, G[3] = {0.0, 0.0, 0.0};
    float pf[3] = {0.f, 0.f, 0.f}, gf[3] = {0.f, 0.f, 0.f};
    if (body) {
        const float* r = a.rb + (int64_t)e * a.rb_env_stride + 13 * lane;
        const float* g = a.ref_pos + (int64_t)e * a.ref_env_stride + 3 * lane;
#pragma unroll
        for (int k = 0; k < 3; ++k) { pf[k] = r[k]; gf[k] = g[k]; P[k] = (double)pf[k]; G[k] = (double)gf[k]; }
    }
    // the ring: slot (s & 1) holds step s - 2 until this launch overwrites it with step s, the other slot holds step s - 1
    float* ring_e = a.ring + (int64_t)e * 12 * J;             // (2 slots, pred | gt, J, 3)
    const int cur = s & 1;
    double P1[3] = {0, 0, 0}, G1[3] = {0, 0, 0}, P2[3] = {0, 0, 0}, G2[3] = {0, 0, 0};
    if (body) {
        float* c_p = ring_e + (cur * 2 + 0) * 3 * J + 3 * lane;
        float* c_g = ring_e + (cur * 2 + 1) * 3 * J + 3 * lane;
        const float* o_p = ring_e + ((1 - cur) * 2 + 0) * 3 * J + 3 * lane;
        const float* o_g = ring_e + ((1 - cur) * 2 + 1) * 3 * J + 3 * lane;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            P2[k] = (double)c_p[k]; G2[k] = (double)c_g[k];
            P1[k] = (double)o_p[k]; G1[k] = (double)o_g[k];
            c_p[k] = pf[k]; c_g[k] = gf[k];
        }
    }
    const int nsteps = a.num_steps[e];
    if (!((int64_t)s < (int64_t)nsteps - 1)) return;          // the reference's [:(i - 1), idx] slices (im_amp.py:283-287)

    const double invJ = 1.0 / (double)J;
    // ---- mpjpe_g, mpjpe_l
    const double t_g = lane_sum<LB>(body ? norm3(P[0] - G[0], P[1] - G[1], P[2] - G[2]) : 0.0) * invJ;
    double P0[3], G0[3];                                      // body 0 of the env, from the group's first lane
#pragma unroll
    for (int k = 0; k < 3; ++k) { P0[k] = __shfl(P[k], 0, LB); G0[k] = __shfl(G[k], 0, LB); }
    double Pt[3], Gt[3];                                      // root-relative
#pragma unroll
    for (int k = 0; k < 3; ++k) { Pt[k] = body ? P[k] - P0[k] : 0.0; Gt[k] = body ? G[k] - G0[k] : 0.0; }
    const double t_l = lane_sum<LB>(norm3(Pt[0] - Gt[0], Pt[1] - Gt[1], Pt[2] - Gt[2])) * invJ;

    // ---- mpjpe_pa: the similarity Procrustes fit of the common p_mpjpe, X = target (gt), Y = predicted, both root-relative
    double muX[3], muY[3], X0[3], Y0[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { muX[k] = lane_sum<LB>(Gt[k]) * invJ; muY[k] = lane_sum<LB>(Pt[k]) * invJ; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { X0[k] = body ? Gt[k] - muX[k] : 0.0; Y0[k] = body ? Pt[k] - muY[k] : 0.0; }
    const double normX = sqrt(lane_sum<LB>(X0[0] * X0[0] + X0[1] * X0[1] + X0[2] * X0[2]));
    const double normY = sqrt(lane_sum<LB>(Y0[0] * Y0[0] + Y0[1] * Y0[1] + Y0[2] * Y0[2]));
    const double invX = normX > 0.0 ? 1.0 / normX : 0.0, invY = normY > 0.0 ? 1.0 / normY : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { X0[k] *= invX; Y0[k] *= invY; }
    double H[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) H[i][k] = lane_sum<LB>(X0[i] * Y0[k]);
    jacobi_svd3(H, V);                                        // H now holds U Sigma, column by column
    double sig[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) sig[i] = norm3(H[0][i], H[1][i], H[2][i]);
    // U: the columns that can be normalised.  One shorter than kRankTol of the longest is what rounding left of a zero singular value: its
    // direction means nothing (dividing it by its length gave a unit vector INSIDE the span of the others), and LAPACK, which the
    // definition rests on, returns an orthonormal U whatever the rank.  So the missing columns are completed (det U = + 1), add nothing to
    // the trace, and R = V D U^T is a rotation for every H: rank 2 fixes it (the out-of-plane part of the other cloud is turned with the
    // rest, not dropped), rank 1 fixes how v_1 goes onto u_1 and leaves the turn about u_1 to the completion, rank 0 gives R = V.
    const double smax = fmax(sig[0], fmax(sig[1], sig[2]));
    bool keep[3];
    double U[3][3];
    int kept = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        keep[i] = sig[i] > kRankTol * smax;
        kept += keep[i] ? 1 : 0;
        const double w = keep[i] ? 1.0 / sig[i] : 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) U[c][i] = H[c][i] * w;
    }
    if (kept < 3) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {                          // k: the only kept column (rank 1); its two successors are built from it
            if (!(kept == 1 && keep[k])) continue;
            const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
            const double a0 = fabs(U[0][k]), a1 = fabs(U[1][k]), a2 = fabs(U[2][k]);
            const int ax = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);                  // the coordinate axis furthest from u_k
            const double ex = ax == 0 ? 1.0 : 0.0, ey = ax == 1 ? 1.0 : 0.0, ez = ax == 2 ? 1.0 : 0.0;
            double t[3] = {U[1][k] * ez - U[2][k] * ey, U[2][k] * ex - U[0][k] * ez, U[0][k] * ey - U[1][k] * ex};
            const double it = 1.0 / norm3(t[0], t[1], t[2]);                                 // |u_k x e| >= sqrt(2 / 3)
#pragma unroll
            for (int c = 0; c < 3; ++c) U[c][k1] = t[c] * it;
            U[0][k2] = U[1][k] * U[2][k1] - U[2][k] * U[1][k1];
            U[1][k2] = U[2][k] * U[0][k1] - U[0][k] * U[2][k1];
            U[2][k2] = U[0][k] * U[1][k1] - U[1][k] * U[0][k1];
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) {                          // m: the only missing column (rank 2) = the cross product of its two successors
            if (!(kept == 2 && !keep[m])) continue;
            const int m1 = (m + 1) % 3, m2 = (m + 2) % 3;
            U[0][m] = U[1][m1] * U[2][m2] - U[2][m1] * U[1][m2];
            U[1][m] = U[2][m1] * U[0][m2] - U[0][m1] * U[2][m2];
            U[2][m] = U[0][m1] * U[1][m2] - U[1][m1] * U[0][m2];
        }
        if (kept == 0) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) U[c][i] = (c == i) ? 1.0 : 0.0;
        }
    }
    // det(V U^T) = det U (det V = + 1; + 1 for a completed U): a reflection flips the column of the SMALLEST singular value (numpy's last).
    // The sign is taken from the orthonormal U, where it is + 1 or - 1 to rounding, not from det H, which is all rounding once H is near singular
    const double detU = U[0][0] * (U[1][1] * U[2][2] - U[1][2] * U[2][1]) - U[0][1] * (U[1][0] * U[2][2] - U[1][2] * U[2][0]) +
                        U[0][2] * (U[1][0] * U[2][1] - U[1][1] * U[2][0]);
    int kmin = 0;
    if (sig[1] < sig[kmin]) kmin = 1;
    if (sig[2] < sig[kmin]) kmin = 2;
    double R[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, tr = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double d = (detU < 0.0 && i == kmin) ? -1.0 : 1.0;
        tr += keep[i] ? d * sig[i] : 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) R[r][c] += V[r][i] * (d * U[c][i]);          // R = V D U^T
    }
    const double scale = tr * normX * invY;
    double tvec[3], al[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) tvec[c] = muX[c] - scale * (muY[0] * R[0][c] + muY[1] * R[1][c] + muY[2] * R[2][c]);
#pragma unroll
    for (int c = 0; c < 3; ++c) al[c] = scale * (Pt[0] * R[0][c] + Pt[1] * R[1][c] + Pt[2] * R[2][c]) + tvec[c];
    const double t_pa = lane_sum<LB>(body ? norm3(al[0] - Gt[0], al[1] - Gt[1], al[2] - Gt[2]) : 0.0) * invJ;

    // ---- vel_dist, accel_dist (finite differences over recorded steps)
    double dv[3], da[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        dv[k] = (P[k] - P1[k]) - (G[k] - G1[k]);
        da[k] = (P[k] - 2.0 * P1[k] + P2[k]) - (G[k] - 2.0 * G1[k] + G2[k]);
    }
    const double t_v = lane_sum<LB>(body ? norm3(dv[0], dv[1], dv[2]) : 0.0) * invJ;
    const double t_a = lane_sum<LB>(body ? norm3(da[0], da[1], da[2]) : 0.0) * invJ;

    if (lane == 0) {
        double* acc = a.accum + (int64_t)e * a.accum_stride;
        acc[0] += 1000.0 * t_g;
        acc[1] += 1000.0 * t_l;
        acc[2] += 1000.0 * t_pa;
        acc[5] += 1.0;
        if (s >= 1) { acc[3] += 1000.0 * t_v; acc[6] += 1.0; }
        if (s >= 2) { acc[4] += 1000.0 * t_a; acc[7] += 1.0; }
    }
}

}  // namespace
}  // namespace pulse

using namespace pulse;

extern "C" int pulse_sizeof_im_eval_args(void) { return (int)sizeof(pulse_im_eval_args); }

extern "C" int pulse_im_eval_accum(const pulse_im_eval_args* args, pulse_stream_t s) {
    PULSE_REQUIRE(args != nullptr, "pulse_im_eval_accum: null args");
    const pulse_im_eval_args& a = *args;
    PULSE_REQUIRE(a.num_envs >= 0, "pulse_im_eval_accum: negative num_envs %d", a.num_envs);
    if (a.num_envs == 0) return PULSE_OK;
    const int J = a.num_bodies;
    PULSE_REQUIRE(J >= 1 && J <= 64, "pulse_im_eval_accum: num_bodies %d not in [1,64]", J);
    PULSE_REQUIRE(a.rb != nullptr, "pulse_im_eval_accum: null rb (the simulated rigid-body records)");
    PULSE_REQUIRE(a.ref_pos != nullptr, "pulse_im_eval_accum: null ref_pos (the reference body positions)");
    PULSE_REQUIRE(a.num_steps != nullptr, "pulse_im_eval_accum: null num_steps");
    PULSE_REQUIRE(a.ring != nullptr, "pulse_im_eval_accum: null ring");
    PULSE_REQUIRE(a.accum != nullptr, "pulse_im_eval_accum: null accum");
    PULSE_REQUIRE(a.step >= 0, "pulse_im_eval_accum: negative step %d", a.step);
    PULSE_REQUIRE(a.rb_env_stride >= 13LL * J, "pulse_im_eval_accum: rb_env_stride %lld is short of the %d floats of %d body records", (long long)a.rb_env_stride, 13 * J, J);
    PULSE_REQUIRE(a.ref_env_stride >= 3LL * J, "pulse_im_eval_accum: ref_env_stride %lld is short of the %d floats of %d positions", (long long)a.ref_env_stride, 3 * J, J);
    PULSE_REQUIRE(a.accum_stride >= 8, "pulse_im_eval_accum: accum_stride %lld is short of the 8 doubles of an accumulator row", (long long)a.accum_stride);
    PULSE_REQUIRE(reinterpret_cast<uintptr_t>(a.rb) % 4 == 0 && reinterpret_cast<uintptr_t>(a.ref_pos) % 4 == 0 && reinterpret_cast<uintptr_t>(a.ring) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(a.num_steps) % 4 == 0, "pulse_im_eval_accum: rb, ref_pos, ring and num_steps must be 4-byte aligned");
    PULSE_REQUIRE(reinterpret_cast<uintptr_t>(a.accum) % 8 == 0, "pulse_im_eval_accum: accum must be 8-byte aligned");
    const bool wide = J > kHalfWave;
    unsigned blocks;
    if (const int rc = lane_group_blocks("pulse_im_eval_accum", a.num_envs, kEvalThreads / (wide ? 64 : 32), blocks)) return rc;
    if (wide) hipLaunchKernelGGL(im_eval_accum_kernel<64>, dim3(blocks), dim3(kEvalThreads), 0, as_stream(s), a);
    else hipLaunchKernelGGL(im_eval_accum_kernel<32>, dim3(blocks), dim3(kEvalThreads), 0, as_stream(s), a);
    return check_launch("pulse_im_eval_accum");
}
