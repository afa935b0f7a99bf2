// The host checks of pulse_amd/csrc/body_lanes.h at the bounds of their fixed-size arrays, as a
// stand-alone host program for AddressSanitizer + UBSan: check_tree, check_permutation, check_record_layout and check_motion_tables at
// J = 1, 2, 32, 33, 64, 65 with a chain tree (depth J - 1) and a star tree; the filled arrays are printed.  Nothing touches a device.
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Ipulse_amd/csrc -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/launch_checks_host.cpp -o tools/launch_checks_host
//   ./tools/launch_checks_host            # exit status 0 and "launch_checks_host: ok" as the last line
#include <cstdio>
#include <cstring>
#include <vector>
#include "body_lanes.h"

namespace pulse {
char* last_error_buf() {
    static thread_local char buf[512];
    return buf;
}
}  // namespace pulse

using namespace pulse;

static int g_wrong = 0;
static void expect(bool ok, const char* what, int J) {
    if (!ok) { ++g_wrong; std::printf("WRONG: %s at J = %d (%s)\n", what, J, last_error_buf()); }
}

template <int MaxB>
static void tree_case(const char* shape, int J) {
    std::vector<int32_t> parents(J);                        // exactly J entries: a read past them is ASan's to find
    for (int b = 0; b < J; ++b) parents[b] = b == 0 ? -1 : (shape[0] == 'c' ? b - 1 : 0);
    struct { unsigned char before[16]; BodyTree<MaxB> tree; unsigned char after[16]; } g;
    std::memset(&g, 0xa5, sizeof g);
    const int rc = check_tree("host", parents.data(), J, g.tree);
    for (int i = 0; i < 16; ++i) expect(g.before[i] == 0xa5 && g.after[i] == 0xa5, "check_tree wrote outside the tree", J);
    if (J > MaxB) {
        expect(rc == PULSE_ERR_INVALID_ARG, "check_tree accepted more bodies than lanes", J);
        std::printf("tree<%d> %s J=%d refused: %s\n", MaxB, shape, J, last_error_buf());
        return;
    }
    expect(rc == PULSE_OK, "check_tree refused a valid tree", J);
    expect(g.tree.max_depth == (J == 1 ? 0 : (shape[0] == 'c' ? J - 1 : 1)), "max_depth", J);
    std::printf("tree<%d> %s J=%d max_depth=%d parent:", MaxB, shape, J, g.tree.max_depth);
    for (int b = 0; b < MaxB; ++b) std::printf(" %d", g.tree.parent[b]);
    std::printf(" depth:");
    for (int b = 0; b < MaxB; ++b) std::printf(" %d", g.tree.depth[b]);
    std::printf("\n");
    for (int b = J; b < MaxB; ++b) expect(g.tree.parent[b] == -1 && g.tree.depth[b] == 0, "bodies past J", J);
}

static void permutation_case(int J) {
    std::vector<int32_t> map(J);
    for (int b = 0; b < J; ++b) map[b] = J - 1 - b;
    struct { unsigned char before[16]; unsigned char inverse[64]; unsigned char after[16]; } g;
    std::memset(&g, 0xa5, sizeof g);
    const int rc = check_permutation<64>("host", "joint_map", map.data(), J, g.inverse);
    for (int i = 0; i < 16; ++i) expect(g.before[i] == 0xa5 && g.after[i] == 0xa5, "check_permutation wrote outside the inverse", J);
    if (J > 64) {
        expect(rc == PULSE_ERR_INVALID_ARG, "check_permutation accepted more bodies than lanes", J);
        std::printf("permutation J=%d refused: %s\n", J, last_error_buf());
        return;
    }
    expect(rc == PULSE_OK && check_permutation<64>("host", "joint_map", map.data(), J, nullptr) == PULSE_OK, "check_permutation refused a permutation", J);
    std::printf("permutation J=%d inverse:", J);
    for (int j = 0; j < J; ++j) { std::printf(" %d", g.inverse[j]); expect(g.inverse[j] == J - 1 - j, "inverse", J); }
    std::printf("\n");
    if (J >= 2) {
        map[J - 1] = map[0];
        expect(check_permutation<64>("host", "joint_map", map.data(), J, nullptr) == PULSE_ERR_INVALID_ARG, "a repeated entry accepted", J);
        map[J - 1] = J;
        expect(check_permutation<64>("host", "joint_map", map.data(), J, nullptr) == PULSE_ERR_INVALID_ARG, "an entry past the end accepted", J);
    }
}

static void layout_case(int J) {
    // [grs | lrs | gts | gvs | gavs | dvs | pad to a multiple of 4]: the layout the package builds
    const int grs = 0, lrs = 4 * J, gts = 8 * J, gvs = 11 * J, gavs = 14 * J, dvs = 17 * J, used = 20 * J - 3;
    const long long stride = (used + 3) / 4 * 4;
    alignas(16) static float frames[4];
    expect(check_record_layout("host", J, stride, gts, grs, lrs, gvs, gavs, dvs, frames) == PULSE_OK, "check_record_layout refused the package's layout", J);
    expect(check_record_layout("host", J, stride, gts, grs, lrs, gvs, gavs, dvs, frames + 1) == PULSE_ERR_INVALID_ARG, "a misaligned base accepted", J);
    expect(check_record_layout("host", J, stride, gts, grs, lrs, gvs, gavs, 0x7fffffff, frames) == PULSE_ERR_INVALID_ARG, "an offset at INT_MAX accepted", J);
    expect(check_record_layout("host", J, stride, gts, grs, lrs, gvs, gvs, dvs, frames) == PULSE_ERR_INVALID_ARG, "overlapping fields accepted", J);
    const float lengths[1] = {1.0f};
    const int64_t counts[1] = {2};
    pulse_motion_tables T = {};
    T.frames = frames; T.frame_stride = stride; T.total_frames = 2; T.num_bodies = J;
    T.off_gts = gts; T.off_grs = grs; T.off_lrs = lrs; T.off_gvs = gvs; T.off_gavs = gavs; T.off_dvs = dvs;
    T.motion_lengths = lengths; T.motion_dt = lengths; T.motion_num_frames = counts; T.length_starts = counts; T.num_motions = 1;
    for (const int most : {32, 64}) {
        const int rc = check_motion_tables("host", T, most);
        expect(rc == (J <= most ? PULSE_OK : PULSE_ERR_INVALID_ARG), "check_motion_tables at the body bound", J);
        std::printf("tables J=%d max=%d stride=%lld: %s\n", J, most, stride, rc == PULSE_OK ? "accepted" : last_error_buf());
    }
    pulse_motion_tables B = T;
    B.off_dvs = 0x7fffffff;
    expect(check_motion_tables("host", B, 64) == PULSE_ERR_INVALID_ARG || J > 64, "an offset at INT_MAX accepted by check_motion_tables", J);
    B = T;
    B.frame_stride = INT64_MIN;
    expect(check_motion_tables("host", B, 64) == PULSE_ERR_INVALID_ARG, "the most negative pitch accepted", J);
}

int main() {
    for (const int J : {1, 2, 32, 33, 64, 65}) {
        for (const char* shape : {"chain", "star"}) {
            tree_case<32>(shape, J);
            tree_case<64>(shape, J);
        }
        permutation_case(J);
        layout_case(J);
    }
    unsigned blocks = 0;
    expect(lane_group_blocks("host", 0, 8, blocks) == PULSE_OK && blocks == 0, "no items", 0);
    expect(lane_group_blocks("host", 9, 8, blocks) == PULSE_OK && blocks == 2, "nine items", 0);
    expect(lane_group_blocks("host", 0x7fffffffLL * 8, 8, blocks) == PULSE_OK && blocks == 0x7fffffffu, "the largest grid", 0);
    expect(lane_group_blocks("host", 0x7fffffffLL * 8 + 1, 8, blocks) == PULSE_ERR_INVALID_ARG, "one item past the largest grid", 0);
    expect(lane_group_blocks("host", INT64_MAX, 8, blocks) == PULSE_ERR_INVALID_ARG, "INT64_MAX items", 0);
    std::printf(g_wrong ? "launch_checks_host: %d WRONG\n" : "launch_checks_host: ok\n", g_wrong);
    return g_wrong ? 1 : 0;
}
