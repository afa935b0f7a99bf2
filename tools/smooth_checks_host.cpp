// The launchers of pulse_amd/csrc/motion_smooth.hip (pulse_motion_euler_pose, pulse_motion_smooth) at the edges of their host checks, as a
// stand-alone host program for AddressSanitizer + UBSan: the translation unit itself is included, every call below is refused before
// anything is launched (or has nothing to do), and nothing touches a device.  Clip tables of exactly M entries, trees of exactly J: a read
// past them is ASan's to find; frame counts up to INT64_MAX: a byte count formed before the grid check would be UBSan's.
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Ipulse_amd/csrc -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/smooth_checks_host.cpp -o tools/smooth_checks_host
//   ./tools/smooth_checks_host            # exit status 0 and "smooth_checks_host: ok" as the last line
#include <cstdio>
#include <cstring>
#include <vector>
#include "../pulse_amd/csrc/motion_smooth.hip"

namespace pulse {
char* last_error_buf() {
    static thread_local char buf[512];
    return buf;
}
}  // namespace pulse

static int g_wrong = 0;
static void refused(int rc, const char* needle, const char* what) {
    const bool ok = rc == PULSE_ERR_INVALID_ARG && std::strstr(pulse::last_error_buf(), needle);
    if (!ok) ++g_wrong;
    std::printf("%s %s: rc %d: %s\n", ok ? "ok   " : "WRONG", what, rc, pulse::last_error_buf());
}

static float* fake(unsigned long long address) { return reinterpret_cast<float*>(static_cast<uintptr_t>(address)); }

int main() {
    for (const int J : {1, 24, 32, 33}) {
        for (const long long first : {3LL, 0LL, 1LL << 35, (long long)INT64_MAX}) {
            std::vector<int64_t> frames = {first, 2};
            std::vector<int32_t> parents(J);
            for (int b = 0; b < J; ++b) parents[b] = b - 1;
            pulse_motion_smooth_args a = {};
            a.in_rot = fake(1ULL << 40); a.in_trans = fake(2ULL << 40); a.out_rot = fake(3ULL << 40); a.out_trans = fake(4ULL << 40);
            a.out_pose_quat = fake(5ULL << 40);
            a.clip_start = reinterpret_cast<const int64_t*>(fake(6ULL << 40)); a.sign_words = reinterpret_cast<uint32_t*>(fake(7ULL << 40));
            a.clip_frames_host = frames.data(); a.parent_indices_host = parents.data();
            a.num_clips = 2; a.num_bodies = J; a.radius_rot = 8; a.radius_trans = 12;
            a.total_frames = first > INT64_MAX - 2 ? first : first + 2;
            char what[96];
            std::snprintf(what, sizeof what, "smooth J=%d frames={%lld, 2}", J, first);
            const int rc = pulse_motion_smooth(&a, nullptr);
            if (J == 33) refused(rc, "num_bodies 33 not in [1,32]", what);
            else if (first == 0) refused(rc, "clip 0 has 0 frames", what);
            else if (first == INT64_MAX) refused(rc, "more frames than total_frames", what);
            else if (first == 1LL << 35) refused(rc, "exceed the grid", what);
            else {                                                   // valid so far: refuse it at the last check before the launch
                a.out_trans = const_cast<float*>(a.in_trans) + 3 * 4;
                refused(pulse_motion_smooth(&a, nullptr), "out_trans overlaps in_trans", what);
                a.out_trans = fake(4ULL << 40);
                a.out_rot = const_cast<float*>(a.in_rot) + 4 * (5LL * J - 1);
                refused(pulse_motion_smooth(&a, nullptr), "out_rot overlaps in_rot", what);
                continue;
            }
            pulse_motion_euler_pose_args e = {};
            e.src_theta = fake(1ULL << 40); e.src_trans = fake(2ULL << 40); e.out_pose = fake(3ULL << 40); e.out_trans = fake(4ULL << 40);
            e.clip_start = a.clip_start; e.clip_frames_host = frames.data(); e.num_clips = 2; e.total_frames = a.total_frames;
            std::snprintf(what, sizeof what, "euler frames={%lld, 2}", first);
            const int rce = pulse_motion_euler_pose(&e, nullptr);
            if (first == 0) refused(rce, "clip 0 has 0 frames", what);
            else if (first == INT64_MAX) refused(rce, "more frames than total_frames", what);
            else if (first == 1LL << 35) refused(rce, "exceed the grid", what);
        }
    }
    pulse_motion_smooth_args none = {};
    pulse_motion_euler_pose_args none_e = {};
    if (pulse_motion_smooth(&none, nullptr) != PULSE_OK || pulse_motion_euler_pose(&none_e, nullptr) != PULSE_OK) { ++g_wrong; std::printf("WRONG: nothing to do refused\n"); }
    refused(pulse_motion_smooth(nullptr, nullptr), "null args", "smooth null");
    refused(pulse_motion_euler_pose(nullptr, nullptr), "null args", "euler null");
    std::printf(g_wrong ? "smooth_checks_host: %d WRONG\n" : "smooth_checks_host: ok\n", g_wrong);
    return g_wrong ? 1 : 0;
}
