// RunningMeanStd on gfx950 (HBM- or latency-bound): rms_normalize / rms_update = RunningMeanStd.forward, phc/utils/running_mean_std.py:56-109,
// fused with the AMPDataset minibatch row gather (phc/learning/amp_datasets.py:81-94).
//
// Statistics are accumulated in fp64 (the reference keeps fp64 running buffers; fp64 partials make the
// batch moments independent of the block decomposition to ~1e-16).  Compiled with -ffp-contract=off.
#include "learner_math.h"

namespace pulse {

// wide matrices (cols >= 64): threads own columns, blocks own row chunks.
constexpr int kRmsMaxColsPerThread = 12;  // 256 threads x 12 = 3072 columns (AMP obs is 10 x 232 = 2320)

__global__ void __launch_bounds__(256) rms_normalize_wide_kernel(const float* __restrict__ x, long long x_stride, const long long* __restrict__ row_idx, int rows,
                                                                int cols, const double* __restrict__ mean, const double* __restrict__ var, float eps, float clip,
                                                                int mode, float* __restrict__ y, long long y_stride, int y_cols, double* __restrict__ partials) {
    const int tid = threadIdx.x;
    const int nblk = gridDim.x, per = (rows + nblk - 1) / nblk, r0 = blockIdx.x * per, r1 = min(rows, r0 + per);      // this workgroup's rows
    float mu[kRmsMaxColsPerThread], den[kRmsMaxColsPerThread];
    double s1[kRmsMaxColsPerThread], s2[kRmsMaxColsPerThread];
#pragma unroll
    for (int j = 0; j < kRmsMaxColsPerThread; ++j) {
        const int c = tid + 256 * j;
        s1[j] = 0.0; s2[j] = 0.0;
        if (c < cols) { mu[j] = (float)mean[c]; den[j] = rms_den(var[c], eps); }
        else { mu[j] = 0.f; den[j] = 1.f; }
    }
    for (int r = r0; r < r1; ++r) {
        const long long src = row_idx ? row_idx[r] : (long long)r;
        const float* xr = x + src * x_stride;
        float* yr = y + (long long)r * y_stride;
#pragma unroll
        for (int j = 0; j < kRmsMaxColsPerThread; ++j) {
            const int c = tid + 256 * j;
            if (c < cols) {
                const float v = xr[c];
                s1[j] += (double)v; s2[j] += (double)v * (double)v;
                yr[c] = rms_apply(v, mu[j], den[j], clip, mode);
            } else if (c < y_cols) {
                yr[c] = 0.f;
            }
        }
    }
    if (partials) {
        double* p = partials + (long long)blockIdx.x * 2 * cols;
#pragma unroll
        for (int j = 0; j < kRmsMaxColsPerThread; ++j) {
            const int c = tid + 256 * j;
            if (c < cols) { p[c] = s1[j]; p[cols + c] = s2[j]; }
        }
    }
}

// 16-byte variant of the wide kernel: each thread owns groups of 4 adjacent columns (a wave reads 1 KiB
// of a row per instruction).  Needs 16-byte aligned rows on both sides and y_cols % 4 == 0.
constexpr int kRmsVecGroups = 3;   // 256 threads x 4 columns x 3 groups = 3072 columns
constexpr int kRmsRowsPerPass = 64;
constexpr int kRmsRowsInFlight = 4;     // rows whose loads are in flight per workgroup (4 KB each): the row loop is a latency x concurrency product

// OUT = 1: besides y, the three bf16 planes of every output element (common.h: split_pair3) go to planes[p * plane_stride + row * planes_ld + col]
// -- the layer-1 operand of the planar GEMM (gemm_x3p.hip) written by its producer instead of a separate split pass.
// OUT = 2: the output IS a bf16 matrix (planes[row * planes_ld + col], y unused): the layer-1 operand of the bf16-storage training path
// (mixed_precision; a bf16 autocast Linear rounds its fp32 input exactly like this).
// G: column groups per thread.  G = 1 (rows of <= 1024 columns: every observation of this path) needs 62 - 70 VGPRs instead of 141 - 146, so
// three workgroups share a CU instead of one and the 512 workgroups of a 16384-row minibatch are resident at once: 28.4 -> 22.0 us for
// 16384 x 934 -> 960 (5.6 TB/s of read + write; eight rows in flight per half instead of four measured 24.9).  [r6]
template <int OUT, int G = kRmsVecGroups>
__global__ void __launch_bounds__(512) rms_normalize_vec4_kernel(const float* __restrict__ x, long long x_stride, const long long* __restrict__ row_idx, int rows,
                                                                int cols, const double* __restrict__ mean, const double* __restrict__ var, float eps, float clip,
                                                                int mode, float* __restrict__ y, long long y_stride, int y_cols, double* __restrict__ partials,
                                                                unsigned short* __restrict__ planes, long long plane_stride, long long planes_ld, float* __restrict__ raw,
                                                                long long raw_stride) {
    // 512 threads = two halves of 256 column owners: the halves take alternate groups of kRmsRowsInFlight rows of the workgroup's row range and
    // their moment sums are combined through LDS at the end.  (One workgroup per CU with four waves could not hide the row loads' latency:
    // 4096 x 1960 rows took 29 us = 1.6 TB/s; the partials per WORKGROUP, which rms_update has to read back, stay what they were.)
    const int tid = threadIdx.x & 255, hf = threadIdx.x >> 8;
    const int nblk = gridDim.x, per = (rows + nblk - 1) / nblk, r0 = blockIdx.x * per, r1 = min(rows, r0 + per);      // this workgroup's rows
    float mu[G][4], den[G][4];
    double s1[G][4], s2[G][4];
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = (tid + 256 * j) * 4 + k;
            s1[j][k] = 0.0; s2[j][k] = 0.0;
            if (c < cols) { mu[j][k] = (float)mean[c]; den[j][k] = rms_den(var[c], eps); }
            else { mu[j][k] = 0.f; den[j][k] = 1.f; }
        }
    // the gather indices of this block's rows go through LDS once (a dependent index load per row would put a full
    // memory latency in front of every row), then rows are processed two at a time so two rows' loads are in flight
    __shared__ long long s_src[kRmsRowsPerPass];
    for (int rb = r0; rb < r1; rb += kRmsRowsPerPass) {
        const int nr = min(kRmsRowsPerPass, r1 - rb);
        __syncthreads();
        if ((int)threadIdx.x < nr) s_src[threadIdx.x] = row_idx ? row_idx[rb + threadIdx.x] : (long long)(rb + threadIdx.x);
        __syncthreads();
        for (int q = hf * kRmsRowsInFlight; q < nr; q += 2 * kRmsRowsInFlight) {
            // kRmsRowsInFlight rows' loads are issued before the first is consumed: a workgroup's row loop is latency-bound
            // (one 3.7 KB row per memory round trip otherwise)
            float4 v[kRmsRowsInFlight][G];
#pragma unroll
            for (int h = 0; h < kRmsRowsInFlight; ++h) {
                const float* xr = x + s_src[q + h < nr ? q + h : q] * x_stride;
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    const int c = (tid + 256 * j) * 4;
                    v[h][j] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (c < cols) v[h][j] = *reinterpret_cast<const float4*>(xr + c);
                }
            }
#pragma unroll
            for (int h = 0; h < kRmsRowsInFlight; ++h) {
                if (q + h >= nr) break;
                float* yr = OUT == 2 ? nullptr : y + (long long)(rb + q + h) * y_stride;
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    const int c = (tid + 256 * j) * 4;
                    if (c < y_cols) {
                        const float4 vv = v[h][j];
                        if (raw && c < cols) *reinterpret_cast<float4*>(raw + (long long)(rb + q + h) * raw_stride + c) = vv;     // the rollout's record of the raw row
                        float in[4] = {vv.x, vv.y, vv.z, vv.w}, o[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            if (c + k < cols) {
                                s1[j][k] += (double)in[k]; s2[j][k] += (double)in[k] * (double)in[k];
                                o[k] = rms_apply(in[k], mu[j][k], den[j][k], clip, mode);
                            } else {
                                o[k] = 0.f;
                            }
                        }
                        if constexpr (OUT == 2) {
                            *reinterpret_cast<uint2*>(planes + (long long)(rb + q + h) * planes_ld + c) = make_uint2(split_pack_rn(o[0], o[1]), split_pack_rn(o[2], o[3]));
                        } else {
                            *reinterpret_cast<float4*>(yr + c) = make_float4(o[0], o[1], o[2], o[3]);
                        }
                        if constexpr (OUT == 1) {
                            unsigned a0, a1, a2, b0, b1, b2;
                            split_pair3(o[0], o[1], a0, a1, a2);
                            split_pair3(o[2], o[3], b0, b1, b2);
                            unsigned short* pr = planes + (long long)(rb + q + h) * planes_ld + c;
                            *reinterpret_cast<uint2*>(pr) = make_uint2(a0, b0);
                            *reinterpret_cast<uint2*>(pr + plane_stride) = make_uint2(a1, b1);
                            *reinterpret_cast<uint2*>(pr + 2 * plane_stride) = make_uint2(a2, b2);
                        }
                    }
                }
            }
        }
    }
    if (partials) {
        __shared__ double s_red[2 * G * 4][256];           // 48 KB: the upper half's sums, [moment, group, column-in-group][owner]
        __syncthreads();
        if (hf == 1) {
#pragma unroll
            for (int j = 0; j < G; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) { s_red[j * 4 + k][tid] = s1[j][k]; s_red[G * 4 + j * 4 + k][tid] = s2[j][k]; }
        }
        __syncthreads();
        if (hf == 0) {
            double* p = partials + (long long)blockIdx.x * 2 * cols;
#pragma unroll
            for (int j = 0; j < G; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = (tid + 256 * j) * 4 + k;
                    if (c < cols) { p[c] = s1[j][k] + s_red[j * 4 + k][tid]; p[cols + c] = s2[j][k] + s_red[G * 4 + j * 4 + k][tid]; }
                }
        }
    }
}

// narrow matrices (cols < 64, e.g. the (B,1) value tensor): threads own rows.
__global__ void __launch_bounds__(256) rms_normalize_narrow_kernel(const float* __restrict__ x, long long x_stride, const long long* __restrict__ row_idx, int rows,
                                                                  int cols, const double* __restrict__ mean, const double* __restrict__ var, float eps, float clip,
                                                                  int mode, float* __restrict__ y, long long y_stride, int y_cols, double* __restrict__ partials) {
    __shared__ double red[2][4];
    const int nblk = gridDim.x, per = (rows + nblk - 1) / nblk, r0 = blockIdx.x * per, r1 = min(rows, r0 + per);      // this workgroup's rows
    for (int c = 0; c < cols; ++c) {
        const float mu = (float)mean[c];
        const float den = rms_den(var[c], eps);
        double s[2] = {0.0, 0.0}, t[2];
        for (int r = r0 + threadIdx.x; r < r1; r += 256) {
            const long long src = row_idx ? row_idx[r] : (long long)r;
            const float v = x[src * x_stride + c];
            s[0] += (double)v; s[1] += (double)v * (double)v;
            y[(long long)r * y_stride + c] = rms_apply(v, mu, den, clip, mode);
        }
        if (partials) {
            block_sum(s, red, t);
            double* p = partials + (long long)blockIdx.x * 2 * cols;
            if (threadIdx.x == 0) { p[c] = t[0]; p[cols + c] = t[1]; }
            __syncthreads();
        }
    }
    for (int r = r0 + threadIdx.x; r < r1; r += 256)
        for (int c = cols; c < y_cols; ++c) y[(long long)r * y_stride + c] = 0.f;
}

__global__ void __launch_bounds__(1024) rms_update_kernel(double* __restrict__ mean, double* __restrict__ var, double* __restrict__ count_out,
                                                        const double* __restrict__ partials, int nblk, int cols, double count, double n) {
    // 16 columns x 64 groups over the partial blocks per workgroup (it was 64 x 16: 15 workgroups for the 934-column policy observation, each
    // walking 32 dependent rounds of loads -- 13 us, latency-bound; 59 workgroups of 8 rounds now).  [r5]
    __shared__ double red[2][64][16];
    const int cl = threadIdx.x & 15, pl = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cl;
    double s1 = 0.0, s2 = 0.0;
    if (c < cols) {
        for (int b = pl; b < nblk; b += 64) {
            s1 += partials[(long long)b * 2 * cols + c];
            s2 += partials[(long long)b * 2 * cols + cols + c];
        }
    }
    red[0][pl][cl] = s1; red[1][pl][cl] = s2;
    __syncthreads();
    if (pl == 0 && c < cols) {
        s1 = 0.0; s2 = 0.0;
#pragma unroll
        for (int g = 0; g < 64; ++g) { s1 += red[0][g][cl]; s2 += red[1][g][cl]; }
        const double bm = s1 / n;
        // unbiased variance like torch.var: sum (x - mean)^2 / (n - 1)
        double bv = (s2 - n * bm * bm) / (n - 1.0);
        if (bv < 0.0) bv = 0.0;
        const double m = mean[c], v = var[c];
        const double delta = bm - m;
        const double tot = count + n;
        const double new_mean = m + delta * n / tot;
        const double m2 = v * count + bv * n + delta * delta * count * n / tot;
        mean[c] = new_mean;
        var[c] = m2 / tot;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && count_out) *count_out = count + n;
}

}  // namespace pulse

using namespace pulse;

namespace {

constexpr int kRmsMaxCols = 256 * 4 * kRmsVecGroups;     // 3072 = 256 * kRmsMaxColsPerThread: what the column owners of the wide kernels reach
static_assert(kRmsMaxCols == 256 * kRmsMaxColsPerThread, "the wide and the vec4 kernel cover the same columns");

// what one normalising call is given, as the four entries share it (y: fp32 or bf16 rows)
struct RmsCall { const char* entry; const float* x; int64_t x_stride; const int64_t* row_idx; int32_t rows, cols; const double *mean, *var; float eps, clip;
                 const void* y; int64_t y_stride; int32_t y_cols; double* partials; int32_t num_blocks; };

// THE wide-row form, what rms_normalize_vec4_kernel can run (after rms_entry_checks): 64 <= cols, y_cols <= 3072 in groups of 4, 16-byte aligned
// input rows that hold cols rounded up to 4, output rows aligned to y_align bytes (16 for fp32 rows, 8 for bf16 rows).  kernels.rms_copy_supported
// is its Python mirror.
bool rms_wide_rows(const RmsCall& c, unsigned y_align) {
    return c.cols >= 64 && c.y_cols <= kRmsMaxCols && (c.x_stride % 4) == 0 && (c.y_stride % 4) == 0 && (c.y_cols % 4) == 0 &&
           (reinterpret_cast<uintptr_t>(c.x) & 15) == 0 && (reinterpret_cast<uintptr_t>(c.y) & (y_align - 1)) == 0 && c.x_stride >= ((c.cols + 3) & ~3);
}

// The checks every normalising entry opens with.  ``pointers``: the entry's own "all there" (its extra output included); ``need_y_align``: the entry needs
// the wide-row form with that output alignment (0: it has kernels for any rows).  Returns PULSE_OK to go on, an error, or kRmsEmpty: nothing to do.
constexpr int kRmsEmpty = 1;
int rms_entry_checks(const RmsCall& c, bool pointers, unsigned need_y_align) {
    PULSE_REQUIRE(c.rows >= 0 && c.cols >= 0, "%s: negative size", c.entry);
    if (c.rows == 0 || c.cols == 0) return kRmsEmpty;
    PULSE_REQUIRE(pointers, "%s: null pointer", c.entry);
    PULSE_REQUIRE(c.num_blocks >= 1, "%s: num_blocks < 1", c.entry);
    // the zero pad [cols, y_cols) is written by the same column owners: a wider pad would stay unwritten
    PULSE_REQUIRE(c.y_cols <= kRmsMaxCols, "%s: y_cols %d > %d (the zero pad is written by the same column owners)", c.entry, c.y_cols, kRmsMaxCols);
    PULSE_REQUIRE(c.y_cols >= c.cols && c.y_stride >= c.y_cols && c.x_stride >= c.cols, "%s: bad pitches", c.entry);
    PULSE_REQUIRE(need_y_align == 0 || rms_wide_rows(c, need_y_align),
                  "%s: needs the wide-row form (64 <= cols, y_cols <= %d, input rows 16-byte and output rows %u-byte aligned)", c.entry, kRmsMaxCols, need_y_align);
    return PULSE_OK;
}

// the wide-row kernel with as many column groups per thread as the row needs (1 / 2 / 3 groups: 62 - 70 / ~100 / 141 - 146 VGPRs)
template <int OUT>
int launch_rms_vec4(const RmsCall& c, int mode, pulse_stream_t s, float* y, unsigned short* planes, long long plane_stride, long long planes_ld, float* raw = nullptr,
                    long long raw_stride = 0) {
    const auto kernel = c.y_cols <= 1024 ? rms_normalize_vec4_kernel<OUT, 1> : c.y_cols <= 2048 ? rms_normalize_vec4_kernel<OUT, 2> : rms_normalize_vec4_kernel<OUT, 3>;
    hipLaunchKernelGGL(kernel, dim3(c.num_blocks), dim3(512), 0, as_stream(s), c.x, (long long)c.x_stride, (const long long*)c.row_idx, c.rows, c.cols, c.mean, c.var,
                       c.eps, c.clip, mode, y, (long long)c.y_stride, c.y_cols, c.partials, planes, plane_stride, planes_ld, raw, raw_stride);
    return check_launch(c.entry);
}

}  // namespace

extern "C" {

int pulse_rms_normalize(const float* x, int64_t x_stride, const int64_t* row_idx, int32_t rows, int32_t cols, const double* mean, const double* var, float eps,
                        float clip, int32_t mode, float* y, int64_t y_stride, int32_t y_cols, double* moment_partials, int32_t num_blocks, pulse_stream_t s) {
    const RmsCall c{"pulse_rms_normalize", x, x_stride, row_idx, rows, cols, mean, var, eps, clip, y, y_stride, y_cols, moment_partials, num_blocks};
    if (const int e = rms_entry_checks(c, x && y && mean && var, 0)) return e == kRmsEmpty ? PULSE_OK : e;
    PULSE_REQUIRE(mode == 0 || mode == 1, "pulse_rms_normalize: bad mode");
    if (rms_wide_rows(c, 16)) return launch_rms_vec4<0>(c, mode, s, y, nullptr, 0LL, 0LL);
    const auto kernel = cols >= 64 ? rms_normalize_wide_kernel : rms_normalize_narrow_kernel;
    hipLaunchKernelGGL(kernel, dim3(num_blocks), dim3(256), 0, as_stream(s), x, (long long)x_stride, (const long long*)row_idx, rows, cols, mean, var, eps, clip, mode, y,
                       (long long)y_stride, y_cols, moment_partials);
    return check_launch(c.entry);
}

int pulse_rms_normalize_copy(const float* x, int64_t x_stride, const int64_t* row_idx, int32_t rows, int32_t cols, const double* mean, const double* var, float eps,
                             float clip, float* y, int64_t y_stride, int32_t y_cols, double* moment_partials, int32_t num_blocks, float* raw_out, int64_t raw_stride,
                             pulse_stream_t s) {
    const RmsCall c{"pulse_rms_normalize_copy", x, x_stride, row_idx, rows, cols, mean, var, eps, clip, y, y_stride, y_cols, moment_partials, num_blocks};
    if (const int e = rms_entry_checks(c, x && y && mean && var && raw_out, 16)) return e == kRmsEmpty ? PULSE_OK : e;
    PULSE_REQUIRE((raw_stride % 4) == 0 && raw_stride >= ((cols + 3) & ~3) && (reinterpret_cast<uintptr_t>(raw_out) & 15) == 0,
                  "pulse_rms_normalize_copy: raw_out rows must be 16-byte aligned and hold cols rounded up to 4 floats");
    return launch_rms_vec4<0>(c, 0, s, y, nullptr, 0LL, 0LL, raw_out, (long long)raw_stride);
}

int pulse_rms_normalize_planes(const float* x, int64_t x_stride, const int64_t* row_idx, int32_t rows, int32_t cols, const double* mean, const double* var, float eps,
                               float clip, float* y, int64_t y_stride, int32_t y_cols, double* moment_partials, int32_t num_blocks, void* planes, int64_t plane_stride,
                               int64_t planes_ld, pulse_stream_t s) {
    const RmsCall c{"pulse_rms_normalize_planes", x, x_stride, row_idx, rows, cols, mean, var, eps, clip, y, y_stride, y_cols, moment_partials, num_blocks};
    if (const int e = rms_entry_checks(c, x && y && mean && var && planes, 16)) return e == kRmsEmpty ? PULSE_OK : e;
    // the planes cover the same y_cols columns as y (columns [cols, y_cols) are written as zeros: the GEMM's k padding)
    PULSE_REQUIRE((y_cols % 32) == 0 && planes_ld >= y_cols && (planes_ld % 8) == 0 && (plane_stride % 8) == 0 && plane_stride >= (int64_t)rows * planes_ld &&
                  (reinterpret_cast<uintptr_t>(planes) & 15) == 0,
                  "pulse_rms_normalize_planes: y_cols must be a multiple of 32 (zero-padded k extent), planes rows 16-byte aligned and covering it");
    return launch_rms_vec4<1>(c, 0, s, y, reinterpret_cast<unsigned short*>(planes), (long long)plane_stride, (long long)planes_ld);
}

int pulse_rms_normalize_b16(const float* x, int64_t x_stride, const int64_t* row_idx, int32_t rows, int32_t cols, const double* mean, const double* var, float eps,
                            float clip, void* y16, int64_t y_stride, int32_t y_cols, double* moment_partials, int32_t num_blocks, pulse_stream_t s) {
    const RmsCall c{"pulse_rms_normalize_b16", x, x_stride, row_idx, rows, cols, mean, var, eps, clip, y16, y_stride, y_cols, moment_partials, num_blocks};
    if (const int e = rms_entry_checks(c, x && y16 && mean && var, 8)) return e == kRmsEmpty ? PULSE_OK : e;
    // the bf16 rows take the planes' slot of the kernel, with the row pitch as their leading dimension
    return launch_rms_vec4<2>(c, 0, s, nullptr, reinterpret_cast<unsigned short*>(y16), 0LL, (long long)y_stride);
}

int pulse_rms_update(double* mean, double* var, double* count_out, const double* moment_partials, int32_t num_blocks, int32_t cols, double count_old, double batch_count,
                     pulse_stream_t s) {
    PULSE_REQUIRE(cols >= 0 && num_blocks >= 1, "pulse_rms_update: bad sizes");
    if (cols == 0) return PULSE_OK;
    PULSE_REQUIRE(mean && var && moment_partials, "pulse_rms_update: null pointer");
    PULSE_REQUIRE(batch_count >= 2.0, "pulse_rms_update: batch of %g rows has no unbiased variance", batch_count);
    hipLaunchKernelGGL(rms_update_kernel, dim3((cols + 15) / 16), dim3(1024), 0, as_stream(s), mean, var, count_out, moment_partials, num_blocks, cols, count_old,
                       batch_count);
    return check_launch("pulse_rms_update");
}
}
