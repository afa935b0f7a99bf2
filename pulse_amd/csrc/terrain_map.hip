// The walkable map of the terrain task for gfx950: where HumanoidPedestrianTerrain may put a humanoid at a reset.
//
// Replaces
//   the poles flagging + ndimage.binary_dilation(iterations=3)   phc/env/tasks/humanoid_pedestrian_terrain.py:1362-1364, 1380, 1443-1445, 1471
//   the valid-cell table of Terrain.__init__                     :1160-1172
//   Terrain.sample_valid_locations                               :1175-1189
//
// The first two run once, at construction, over the whole map (2000 x 5000 cells at the shipped layout): they are written for being right,
// one thread per cell and one workgroup per row, with no tiling.  The third runs on every rollout step behind the reset mask: a gather of
// two floats per env.
// -ffp-contract=off: the keep test and the group formula follow the reference's float32 operation order.
#include "common.h"
#include "env_select.h"

namespace pulse {

constexpr int kRowThreads = 256;                     // workgroup of the per-row kernels: four waves

// ---- obstacle field + dilation -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool terrain_obstacle(const pulse_terrain_walkable_args& a, int r, int c) {
    const int64_t cell = (int64_t)r * a.cols + c;
    if (a.obstacle_mask && a.obstacle_mask[cell]) return true;
    if (!a.tile_flags) return false;
    const int rr = r - a.border, cc = c - a.border;
    if (rr < 0 || cc < 0) return false;
    const int ti = rr / a.length_px, tj = cc / a.width_px;
    if (ti >= a.tile_rows || tj >= a.tile_cols) return false;
    return a.tile_flags[ti * a.tile_cols + tj] != 0 && a.heights[cell] != 0;
}

__global__ void __launch_bounds__(256) terrain_walkable_kernel(const pulse_terrain_walkable_args a) {
    const int per_row = (a.cols + 255) / 256;                                             // workgroups per map row
    const int r = blockIdx.x / per_row, c = (blockIdx.x % per_row) * 256 + threadIdx.x;
    if (c >= a.cols || r >= a.rows) return;
    const int k = a.iterations;
    bool hit = false;
    for (int dr = -k; dr <= k && !hit; ++dr) {
        const int rr = r + dr;
        if (rr < 0 || rr >= a.rows) continue;
        const int w = k - (dr < 0 ? -dr : dr);
        const int c0 = max(c - w, 0), c1 = min(c + w, a.cols - 1);
        for (int cc = c0; cc <= c1; ++cc)
            if (terrain_obstacle(a, rr, cc)) { hit = true; break; }
    }
    a.walkable[(int64_t)r * a.cols + c] = hit ? 1 : 0;
}

// ---- valid-cell table ----------------------------------------------------------------------------------------------------------------------
// row_extents: [2 r] / [2 r + 1] = the first / last candidate column of row r (cols / -1 when it has none); the last four ints are
// xmin, xmax, ymin, ymax over the candidates (rows / -1 / cols / -1 when there is none at all).
__global__ void __launch_bounds__(kRowThreads) terrain_row_extents_kernel(const pulse_terrain_valid_args a) {
    __shared__ int s_lo[kRowThreads / kWave], s_hi[kRowThreads / kWave];
    const int r = blockIdx.x, tid = threadIdx.x;
    const uint8_t* w = a.walkable + (int64_t)r * a.cols;
    int lo = a.cols, hi = -1;
    for (int c = tid; c < a.cols; c += kRowThreads)
        if (w[c] == 0) { lo = min(lo, c); hi = max(hi, c); }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o, kWave)); hi = max(hi, __shfl_xor(hi, o, kWave)); }
    if ((tid & (kWave - 1)) == 0) { s_lo[tid / kWave] = lo; s_hi[tid / kWave] = hi; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < kRowThreads / kWave; ++i) { lo = min(lo, s_lo[i]); hi = max(hi, s_hi[i]); }
        a.row_extents[2 * r] = lo;
        a.row_extents[2 * r + 1] = hi;
    }
}

__global__ void __launch_bounds__(kRowThreads) terrain_bounds_kernel(const pulse_terrain_valid_args a) {
    __shared__ int s_v[4][kRowThreads / kWave];
    const int tid = threadIdx.x;
    int xmin = a.rows, xmax = -1, ymin = a.cols, ymax = -1;
    for (int r = tid; r < a.rows; r += kRowThreads) {
        const int lo = a.row_extents[2 * r], hi = a.row_extents[2 * r + 1];
        if (hi >= 0) { xmin = min(xmin, r); xmax = max(xmax, r); ymin = min(ymin, lo); ymax = max(ymax, hi); }
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        xmin = min(xmin, __shfl_xor(xmin, o, kWave)); xmax = max(xmax, __shfl_xor(xmax, o, kWave));
        ymin = min(ymin, __shfl_xor(ymin, o, kWave)); ymax = max(ymax, __shfl_xor(ymax, o, kWave));
    }
    if ((tid & (kWave - 1)) == 0) { const int wv = tid / kWave; s_v[0][wv] = xmin; s_v[1][wv] = xmax; s_v[2][wv] = ymin; s_v[3][wv] = ymax; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < kRowThreads / kWave; ++i) {
            xmin = min(xmin, s_v[0][i]); xmax = max(xmax, s_v[1][i]); ymin = min(ymin, s_v[2][i]); ymax = max(ymax, s_v[3][i]);
        }
        int* b = a.row_extents + 2 * (int64_t)a.rows;
        b[0] = xmin; b[1] = xmax; b[2] = ymin; b[3] = ymax;
    }
}

struct TerrainKeep {
    float x_hi, x_lo, y_hi, y_lo, scale;             // xmax_s - b, xmin_s + b, ymax_s - b, ymin_s + b
    bool any;
    __device__ __forceinline__ bool row(int r) const { const float x = (float)r * scale; return any && x < x_hi && x > x_lo; }
    __device__ __forceinline__ bool col(int c) const { const float y = (float)c * scale; return y < y_hi && y > y_lo; }
};

__device__ __forceinline__ TerrainKeep terrain_keep_of(const pulse_terrain_valid_args& a) {
    const int* b = a.row_extents + 2 * (int64_t)a.rows;
    TerrainKeep k;
    k.scale = a.horizontal_scale;
    k.any = b[1] >= 0;
    k.x_hi = (float)b[1] * k.scale - a.border_scaled;
    k.x_lo = (float)b[0] * k.scale + a.border_scaled;
    k.y_hi = (float)b[3] * k.scale - a.border_scaled;
    k.y_lo = (float)b[2] * k.scale + a.border_scaled;
    return k;
}

// counts of the kept cells per row into row_offsets[r] (scanned in place by the next kernel)
__global__ void __launch_bounds__(kRowThreads) terrain_row_count_kernel(const pulse_terrain_valid_args a) {
    __shared__ int s_n[kRowThreads / kWave];
    const int r = blockIdx.x, tid = threadIdx.x;
    const TerrainKeep k = terrain_keep_of(a);
    const uint8_t* w = a.walkable + (int64_t)r * a.cols;
    int n = 0;
    if (k.row(r))
        for (int c = tid; c < a.cols; c += kRowThreads) n += (w[c] == 0 && k.col(c)) ? 1 : 0;
    n = lane_sum(n);
    if ((tid & (kWave - 1)) == 0) s_n[tid / kWave] = n;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < kRowThreads / kWave; ++i) n += s_n[i];
        a.row_offsets[r] = n;
    }
}

// exclusive scan of row_offsets[0 .. rows) in place, the total to row_offsets[rows] and *count: one workgroup walks the rows in chunks
__global__ void __launch_bounds__(kRowThreads) terrain_scan_kernel(const pulse_terrain_valid_args a) {
    __shared__ long long s_w[kRowThreads / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    long long carry = 0;
    for (int r0 = 0; r0 < a.rows; r0 += kRowThreads) {
        const int r = r0 + tid;
        const long long v = r < a.rows ? (long long)a.row_offsets[r] : 0;
        long long inc = v;                                                                // inclusive prefix inside the wave
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const long long up = __shfl_up(inc, o, kWave);
            if (lane >= o) inc += up;
        }
        if (lane == kWave - 1) s_w[wv] = inc;
        __syncthreads();
        long long before = 0, total = 0;
        for (int i = 0; i < kRowThreads / kWave; ++i) { if (i < wv) before += s_w[i]; total += s_w[i]; }
        if (r < a.rows) a.row_offsets[r] = carry + before + (inc - v);
        carry += total;
        __syncthreads();                                                                  // s_w is rewritten by the next chunk
    }
    if (tid == 0) { a.row_offsets[a.rows] = carry; *a.count = carry; }
}

// one workgroup per row: the kept cells in column order.  A chunk of 256 columns at a time: the position of a kept cell inside its wave is
// the number of kept lanes below it (ballot + popcount), the waves' totals go through LDS, the chunks' through a running count.
__global__ void __launch_bounds__(kRowThreads) terrain_row_write_kernel(const pulse_terrain_valid_args a) {
    __shared__ int s_n[kRowThreads / kWave];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const TerrainKeep k = terrain_keep_of(a);
    if (!k.row(r)) return;                                                                // (the whole workgroup: r is uniform)
    const uint8_t* w = a.walkable + (int64_t)r * a.cols;
    const float x = (float)r * k.scale;
    long long at = a.row_offsets[r];
    for (int c0 = 0; c0 < a.cols; c0 += kRowThreads) {
        const int c = c0 + tid;
        const bool keep = c < a.cols && w[c] == 0 && k.col(c);
        const unsigned long long m = __ballot(keep);
        const int below = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_n[wv] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int i = 0; i < kRowThreads / kWave; ++i) { if (i < wv) before += s_n[i]; total += s_n[i]; }
        const long long o = at + before + below;
        if (keep && o < a.capacity) { a.coord_x[o] = x; a.coord_y[o] = (float)c * k.scale; }
        at += total;
        __syncthreads();                                                                  // s_n is rewritten by the next chunk
    }
}

// ---- the reset draw ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) terrain_sample_kernel(const pulse_terrain_sample_args a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (!env_enabled(a, e)) return;
    float x, y;
    if (a.group_num_people > 0) {
        const int g = e / a.group_num_people, num_groups = a.num_envs / a.group_num_people;
        const float cx = a.extent_x * a.u_center[g], cy = a.extent_y * a.u_center[num_groups + g];
        const float dx = 16.0f * a.u_dx[e] + -8.0f, dy = -16.0f * a.u_dy[e] + 8.0f;
        x = cx + dx; y = cy + dy;
    } else {
        const long long i = a.idx[e];
        if (i < 0 || i >= a.num_samples) return;
        x = a.coord_x[i]; y = a.coord_y[i];
    }
    a.out[2 * (int64_t)e] = x;
    a.out[2 * (int64_t)e + 1] = y;
}

}  // namespace pulse

using namespace pulse;

extern "C" {

int pulse_sizeof_terrain_walkable_args(void) { return (int)sizeof(pulse_terrain_walkable_args); }
int pulse_sizeof_terrain_valid_args(void) { return (int)sizeof(pulse_terrain_valid_args); }
int pulse_sizeof_terrain_sample_args(void) { return (int)sizeof(pulse_terrain_sample_args); }

int pulse_terrain_walkable(const pulse_terrain_walkable_args* args, pulse_stream_t s) {
    PULSE_REQUIRE(args != nullptr, "pulse_terrain_walkable: null args");
    const pulse_terrain_walkable_args& a = *args;
    PULSE_REQUIRE(a.rows >= 0 && a.cols >= 0, "pulse_terrain_walkable: negative map size");
    if (a.rows == 0 || a.cols == 0) return PULSE_OK;
    const int64_t groups = (int64_t)a.rows * ((a.cols + 255) / 256);
    PULSE_REQUIRE(groups <= 0x7fffffffLL, "pulse_terrain_walkable: map too large for one launch");
    PULSE_REQUIRE(a.iterations >= 0 && a.iterations <= PULSE_TERRAIN_MAX_DILATION,
                  "pulse_terrain_walkable: iterations must be 0 .. %d, got %d", PULSE_TERRAIN_MAX_DILATION, a.iterations);
    PULSE_REQUIRE(a.walkable, "pulse_terrain_walkable: null walkable");
    PULSE_REQUIRE(a.tile_flags || a.obstacle_mask, "pulse_terrain_walkable: neither tile_flags nor obstacle_mask");
    if (a.tile_flags) {
        PULSE_REQUIRE(a.heights, "pulse_terrain_walkable: tile_flags need heights");
        PULSE_REQUIRE(a.tile_rows >= 1 && a.tile_cols >= 1 && a.length_px >= 1 && a.width_px >= 1 && a.border >= 0,
                      "pulse_terrain_walkable: bad tile grid (tile_rows %d, tile_cols %d, length_px %d, width_px %d, border %d)",
                      a.tile_rows, a.tile_cols, a.length_px, a.width_px, a.border);
    }
    hipLaunchKernelGGL(terrain_walkable_kernel, dim3((unsigned)groups), dim3(256), 0, as_stream(s), a);
    return check_launch("pulse_terrain_walkable");
}

int pulse_terrain_valid_cells(const pulse_terrain_valid_args* args, pulse_stream_t s) {
    PULSE_REQUIRE(args != nullptr, "pulse_terrain_valid_cells: null args");
    const pulse_terrain_valid_args& a = *args;
    PULSE_REQUIRE(a.rows >= 0 && a.cols >= 0, "pulse_terrain_valid_cells: negative map size");
    if (a.rows == 0 || a.cols == 0) return PULSE_OK;
    PULSE_REQUIRE(a.walkable && a.row_extents && a.row_offsets && a.count, "pulse_terrain_valid_cells: null pointer");
    PULSE_REQUIRE(a.capacity >= 0 && (a.capacity == 0 || (a.coord_x && a.coord_y)), "pulse_terrain_valid_cells: bad output table");
    PULSE_REQUIRE(a.horizontal_scale > 0.f && a.border_scaled >= 0.f, "pulse_terrain_valid_cells: bad scales");
    const dim3 rows((unsigned)a.rows), one(1), wg(kRowThreads);
    hipLaunchKernelGGL(terrain_row_extents_kernel, rows, wg, 0, as_stream(s), a);
    hipLaunchKernelGGL(terrain_bounds_kernel, one, wg, 0, as_stream(s), a);
    hipLaunchKernelGGL(terrain_row_count_kernel, rows, wg, 0, as_stream(s), a);
    hipLaunchKernelGGL(terrain_scan_kernel, one, wg, 0, as_stream(s), a);
    if (a.capacity > 0) hipLaunchKernelGGL(terrain_row_write_kernel, rows, wg, 0, as_stream(s), a);
    return check_launch("pulse_terrain_valid_cells");
}

int pulse_terrain_sample(const pulse_terrain_sample_args* args, pulse_stream_t s) {
    PULSE_REQUIRE(args != nullptr, "pulse_terrain_sample: null args");
    const pulse_terrain_sample_args& a = *args;
    PULSE_REQUIRE(a.num_envs >= 0, "pulse_terrain_sample: negative num_envs");
    if (a.num_envs == 0) return PULSE_OK;
    PULSE_REQUIRE(a.out, "pulse_terrain_sample: null out");
    PULSE_REQUIRE(a.group_num_people >= 0, "pulse_terrain_sample: negative group_num_people");
    if (a.group_num_people > 0) {
        PULSE_REQUIRE(a.num_envs % a.group_num_people == 0, "pulse_terrain_sample: num_envs %d is not a multiple of group_num_people %d",
                      a.num_envs, a.group_num_people);
        PULSE_REQUIRE(a.u_center && a.u_dx && a.u_dy, "pulse_terrain_sample: group mode needs u_center, u_dx and u_dy");
    } else {
        PULSE_REQUIRE(a.num_samples >= 1, "pulse_terrain_sample: empty table (num_samples must be >= 1)");
        PULSE_REQUIRE(a.coord_x && a.coord_y && a.idx, "pulse_terrain_sample: table mode needs coord_x, coord_y and idx");
    }
    hipLaunchKernelGGL(terrain_sample_kernel, dim3((unsigned)((a.num_envs + 63) / 64)), dim3(64), 0, as_stream(s), a);
    return check_launch("pulse_terrain_sample");
}
}
