// What the body-lane kernels share: LB = 32 or 64 adjacent lanes per item (frame, query or env), lane = body -- the mapping and its grid, the cross-lane
// read inside a half-wave, a quaternion in memory as a float4 -- and what their launchers check on the host before anything is launched (``what`` is the
// entry point's name; the result is PULSE_OK or fail()'s): the skeleton tree, a joint permutation, the fields of a packed frame record, a pulse_motion_tables.
#pragma once
#include "common.h"
#include "rot_math.h"

namespace pulse {

constexpr int kHalfWave = 32;
// group ``slot`` of the workgroup stands for ``item`` (the kernel compares it with its count); Threads / LB items per workgroup
template <int LB, int Threads = 256> struct LaneGroup {
    static constexpr int threads = Threads, slots = Threads / LB;
    int slot, lane;
    long long item;
};
template <int LB, int Threads = 256> __device__ __forceinline__ LaneGroup<LB, Threads> lane_group() {
    const int slot = threadIdx.x / LB, lane = threadIdx.x % LB;
    return {slot, lane, (long long)blockIdx.x * (Threads / LB) + slot};
}
// the grid of ``items`` groups, ``slots`` (LaneGroup::slots) to a workgroup
inline int lane_group_blocks(const char* what, long long items, int slots, unsigned& blocks) {
    const long long n = items <= 0 ? 0 : (items - 1) / slots + 1;
    PULSE_REQUIRE(n <= 0x7fffffffLL, "%s: %lld items exceed the grid (2^31 - 1 workgroups of %d)", what, items, slots);
    blocks = (unsigned)n;
    return PULSE_OK;
}
// a vector / quaternion from another lane of the 32-lane half-wave (every lane of the wave must execute it)
__device__ __forceinline__ V3 lane_read(const V3 v, const int lane) { return V3{__shfl(v.x, lane, kHalfWave), __shfl(v.y, lane, kHalfWave), __shfl(v.z, lane, kHalfWave)}; }
__device__ __forceinline__ Q4 lane_read(const Q4 q, const int lane) { return Q4{__shfl(q.x, lane, kHalfWave), __shfl(q.y, lane, kHalfWave), __shfl(q.z, lane, kHalfWave), __shfl(q.w, lane, kHalfWave)}; }
// a quaternion in memory as one 16-byte access (the launchers check the alignment)
__device__ __forceinline__ Q4 load_q4(const float* p) { const float4 v = *reinterpret_cast<const float4*>(p); return Q4{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ void store_q4(float* p, const Q4 q) { *reinterpret_cast<float4*>(p) = make_float4(q.x, q.y, q.z, q.w); }

// the tree, by value in the kernel arguments (from the launcher's validated host copy); bodies >= J: parent -1, depth 0
template <int MaxB> struct BodyTree { signed char parent[MaxB]; unsigned char depth[MaxB]; int max_depth; };
template <int MaxB> int check_tree(const char* what, const int32_t* parents, int J, BodyTree<MaxB>& tree) {
    PULSE_REQUIRE(J >= 1 && J <= MaxB, "%s: num_bodies %d not in [1,%d]", what, J, MaxB);
    PULSE_REQUIRE(parents != nullptr, "%s: null parent_indices_host", what);
    tree.max_depth = 0;
    for (int b = 0; b < MaxB; ++b) { tree.parent[b] = -1; tree.depth[b] = 0; }
    PULSE_REQUIRE(parents[0] == -1, "%s: body 0 must be the root (parent -1), got parent %d", what, parents[0]);
    for (int b = 1; b < J; ++b) {
        const int p = parents[b];
        PULSE_REQUIRE(p >= 0 && p < b, "%s: parent_indices[%d] = %d: every parent must precede its child (0 <= parent < child)", what, b, p);
        tree.parent[b] = (signed char)p;
        tree.depth[b] = (unsigned char)(tree.depth[p] + 1);
        if (tree.depth[b] > tree.max_depth) tree.max_depth = tree.depth[b];
    }
    return PULSE_OK;
}
// map[0 .. J) is a permutation of 0 .. J - 1; inverse (MaxB entries, if wanted): inverse[map[b]] = b
template <int MaxB> int check_permutation(const char* what, const char* field, const int32_t* map, int J, unsigned char* inverse) {
    PULSE_REQUIRE(J >= 1 && J <= MaxB, "%s: num_bodies %d not in [1,%d]", what, J, MaxB);
    bool seen[MaxB] = {};
    for (int b = 0; b < J; ++b) {
        const int j = map[b];
        PULSE_REQUIRE(j >= 0 && j < J, "%s: %s[%d] = %d is no SMPL joint (0 .. %d)", what, field, b, j, J - 1);
        PULSE_REQUIRE(!seen[j], "%s: %s[%d] = %d is taken twice: %s must be a permutation of 0 .. %d", what, field, b, j, field, J - 1);
        seen[j] = true;
        if (inverse) inverse[j] = (unsigned char)b;
    }
    return PULSE_OK;
}
// the six fields {grs, lrs, gts, gvs, gavs, dvs} of a J-body frame record as every reader needs them: quaternion fields, the pitch and the base on 16-byte
// boundaries, every field inside the pitch
inline int field_width(int i, int J) { return (i < 2 ? 4 : 3) * (i < 5 ? J : J - 1); }
inline int check_record_fields(const char* what, int J, long long stride, const int (&off)[6], const float* frames) {
    const char* const name[7] = {"frame_stride", "off_grs", "off_lrs", "off_gts", "off_gvs", "off_gavs", "off_dvs"};
    const long long quad[3] = {stride, off[0], off[1]};
    for (int i = 0; i < 3; ++i)
        PULSE_REQUIRE(quad[i] % 4 == 0, "%s: %s %lld is no multiple of 4 floats: the record pitch and the quaternion fields must start on 16-byte boundaries", what, name[i], quad[i]);
    for (int i = 0; i < 6; ++i) {
        PULSE_REQUIRE(off[i] >= 0, "%s: negative field offset (%s %d)", what, name[i + 1], off[i]);
        PULSE_REQUIRE((long long)off[i] + field_width(i, J) <= stride, "%s: %s %d: its %d floats end past frame_stride %lld", what, name[i + 1], off[i], field_width(i, J), stride);
    }
    PULSE_REQUIRE(reinterpret_cast<uintptr_t>(frames) % 16 == 0, "%s: frames (the record base) must be 16-byte aligned", what);
    return PULSE_OK;
}
// the producer's rule on top (pulse_motion_build): the fields tile [0, 20 J - 3) without overlap
inline int check_record_layout(const char* what, int J, long long stride, int off_gts, int off_grs, int off_lrs, int off_gvs, int off_gavs, int off_dvs, const float* frames) {
    const int off[6] = {off_grs, off_lrs, off_gts, off_gvs, off_gavs, off_dvs}, used = 20 * J - 3;
    if (const int rc = check_record_fields(what, J, stride, off, frames)) return rc;
    for (int i = 0; i < 6; ++i) {
        const int wi = field_width(i, J);
        PULSE_REQUIRE((long long)off[i] + wi <= used, "%s: field offset %d (width %d) outside the %d floats a %d-body record uses", what, off[i], wi, used, J);
        for (int k = 0; k < i; ++k)
            PULSE_REQUIRE(wi == 0 || field_width(k, J) == 0 || off[i] + wi <= off[k] || off[k] + field_width(k, J) <= off[i], "%s: record fields at offsets %d and %d overlap", what, off[k], off[i]);
    }
    return PULSE_OK;
}
// what every consumer of a pulse_motion_tables depends on: the pointers, a clip to index, one lane per body, the record fields
inline int check_motion_tables(const char* what, const pulse_motion_tables& T, int max_bodies) {
    const void* const ptr[5] = {T.frames, T.motion_lengths, T.motion_dt, T.motion_num_frames, T.length_starts};
    const char* const ptr_name[5] = {"frames", "motion_lengths", "motion_dt", "motion_num_frames", "length_starts"};
    for (int i = 0; i < 5; ++i) PULSE_REQUIRE(ptr[i] != nullptr, "%s: null table pointer (%s)", what, ptr_name[i]);
    PULSE_REQUIRE(T.num_motions >= 1, "%s: num_motions %d: the motion tables hold no clip", what, T.num_motions);
    PULSE_REQUIRE(T.num_bodies >= 1 && T.num_bodies <= max_bodies, "%s: num_bodies %d not in [1,%d]", what, T.num_bodies, max_bodies);
    const int off[6] = {T.off_grs, T.off_lrs, T.off_gts, T.off_gvs, T.off_gavs, T.off_dvs};
    return check_record_fields(what, T.num_bodies, T.frame_stride, off, T.frames);
}

}  // namespace pulse
