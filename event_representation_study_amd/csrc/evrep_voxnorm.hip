// evrep_voxnorm.hip -- the last step of ev-licious' events_to_voxel_grid (ev-licious/src/evlicious/tools/utils.py:77-83, the numpy
// variant) for the B windows of a batch: the channel-last grids of k_voxel (mode 2, float64) or k_voxel_subpixel (float32) become
// the channel-first float32 tensor (B, bins, H, W), standardised over each window's non-zero entries.  Per window, with
// v = (float)grid value:
//     n = #{v != 0};  mean = (sum_nz v) / n;  std = sqrt((sum_nz (v - mean)^2) / n)      (float64; two passes, population form)
//     n > 0 and std > 0:  out = (float)(((double)v - mean) / (1e-5 + std)) where v != 0, +0 elsewhere;  else out = v.
// Three launches; a window of N = H * W * bins values is read as GROUPS of 16 bytes (two float64 / four float32; as one 16-byte
// load where every window starts on a 16-byte boundary, element by element in the same grouping otherwise):
//   k_voxnorm_sum     grid (slices, B).  A workgroup sweeps one slice -- a contiguous run of `slice_groups` groups -- every thread
//                     adding its groups in ascending order (group tid, tid + 256, ...), then the lanes of a wave by a butterfly,
//                     then the four waves in order.  One (count, sum) partial per (window, slice).
//   k_voxnorm_sqdev   grid (slices, B).  Every workgroup folds its window's partials IN SLICE ORDER to n and mean (wave-uniform),
//                     then forms the partial of sum (v - mean)^2 of its slice the same way.  Slice 0 leaves n and mean behind.
//   k_voxnorm_write   grid (<= kWriteBlocks, B).  Folds the second partials in slice order to std.  Then tiles of kTilePx
//                     consecutive pixels: their kTilePx * bins source values are contiguous, are converted on the way into LDS and
//                     leave as `bins` runs of kTilePx consecutive floats, one per channel plane.  Workgroup 0 of a window writes
//                     its statistics.
// The slices depend on (H, W, bins) and the input dtype alone and nothing is added atomically, so a window's result has the same
// bits in every call, alone and at any place of any batch.  No launch reads a size on the host or waits for the device.
#pragma once
#include "evrep_common.h"

namespace evrep {

constexpr int kTilePx = 256;             // pixels of a k_voxnorm_write tile: a run of 1 KiB per channel plane
constexpr int kWriteBlocks = 128;        // workgroups of k_voxnorm_write per window at most (they stride over the tiles)
constexpr int kMaxSlices = 128;          // partials a workgroup folds at most
constexpr uint32_t kMinSliceGroups = 8192;   // 128 KiB, 32 16-byte loads per thread (measured, 32 windows of 304x240x5 float64: 79 us
                                             // at 2048, 66 us at 4096, 63 us at 8192 -- fewer partials to fold per workgroup; 640x480 unchanged)
// LDS words of a tile: element e lives at e + e / 32, so the channel-plane reads (stride `bins` words) spread over the banks for
// the even bin counts too (bins = 16: lanes p and p + 2 would meet on one bank without the shift)
constexpr int kStageWords = kTilePx * EVREP_MAX_CHANNELS + kTilePx * EVREP_MAX_CHANNELS / 32;
static_assert(kTilePx % 4 == 0, "a tile starts on a group boundary for every bin count");
static_assert(kTilePx == kThreads, "k_voxnorm_write: one pixel per thread and channel");

// groups of a slice for a window of `groups` groups: a multiple of kThreads, at most kMaxSlices slices
__host__ __device__ inline uint32_t voxnorm_slice_groups(uint32_t groups) {
    uint32_t per = (groups + kMaxSlices - 1) / kMaxSlices;
    if (per < kMinSliceGroups) per = kMinSliceGroups;
    return (per + kThreads - 1) / kThreads * kThreads;
}

struct VoxnormArgs {
    const void *grid;            // (B, H, W, bins)
    float *out;                  // (B, bins, H, W)
    double *stats;               // [B][4] or null
    double *sum1, *sum2;         // [B][slices]: sum v, sum (v - mean)^2 over the non-zero values of a slice
    uint32_t *cnt;               // [B][slices]: non-zero values of a slice
    double *head;                // [B][2]: n, mean of a window (k_voxnorm_sqdev -> k_voxnorm_write)
    uint32_t N, groups, slice_groups, slices;    // values and groups of a window
    uint32_t HW, bins, tiles;
    uint32_t normalize;
};

template <typename T> struct VoxGroup { static constexpr int V = 16 / (int)sizeof(T); };

// group g of a window as float32 values; past the window's end: 0, which no sum counts
template <typename T, bool VEC>
__device__ inline void voxnorm_load(const T *__restrict__ win, uint32_t g, uint32_t N, float (&v)[VoxGroup<T>::V]) {
    constexpr int V = VoxGroup<T>::V;
    if constexpr (VEC) {
        const uint4 q = gload16(win + (size_t)g * V);
        if constexpr (V == 2) {
            v[0] = (float)__hiloint2double((int)q.y, (int)q.x);
            v[1] = (float)__hiloint2double((int)q.w, (int)q.z);
        } else {
            v[0] = __uint_as_float(q.x); v[1] = __uint_as_float(q.y); v[2] = __uint_as_float(q.z); v[3] = __uint_as_float(q.w);
        }
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const uint32_t i = g * V + k;
            v[k] = i < N ? (float)win[i] : 0.0f;
        }
    }
}

// the sum over a workgroup in a fixed order: lanes by a butterfly (every lane ends with the same bits: a + b == b + a), the
// waves in ascending order.  tmp: kWaves doubles of LDS.  The result is valid in thread 0.  Contains __syncthreads().
__device__ inline double voxnorm_block_sum(double s, double *tmp) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = s;
    __syncthreads();
    double r = tmp[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r += tmp[w];
    __syncthreads();
    return r;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void k_voxnorm_sum(const VoxnormArgs a) {
    constexpr int V = VoxGroup<T>::V;
    __shared__ double tmp[kWaves];
    __shared__ uint32_t scan_tmp[kWaves];
    const uint32_t b = blockIdx.y, slice = blockIdx.x;
    const T *win = static_cast<const T *>(a.grid) + (size_t)b * a.N;
    const uint32_t g0 = slice * a.slice_groups;
    const uint32_t g1 = g0 + a.slice_groups < a.groups ? g0 + a.slice_groups : a.groups;
    uint32_t n = 0;
    double s = 0.0;
#pragma unroll 4
    for (uint32_t g = g0 + threadIdx.x; g < g1; g += kThreads) {
        float v[V];
        voxnorm_load<T, VEC>(win, g, a.N, v);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const bool nz = v[k] != 0.0f;
            n += nz ? 1u : 0u;
            s += nz ? (double)v[k] : 0.0;
        }
    }
    uint32_t n_tot;
    block_exclusive_scan(n, scan_tmp, &n_tot);
    const double s_tot = voxnorm_block_sum(s, tmp);
    if (threadIdx.x == 0) {
        a.cnt[(size_t)b * a.slices + slice] = n_tot;
        a.sum1[(size_t)b * a.slices + slice] = s_tot;
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void k_voxnorm_sqdev(const VoxnormArgs a) {
    constexpr int V = VoxGroup<T>::V;
    __shared__ double tmp[kWaves];
    const uint32_t b = blockIdx.y, slice = blockIdx.x;
    const T *win = static_cast<const T *>(a.grid) + (size_t)b * a.N;
    // n and mean of the window: the same loads and additions in every thread of every workgroup of the window
    const uint32_t *__restrict__ cnt = a.cnt + (size_t)b * a.slices;
    const double *__restrict__ sum1 = a.sum1 + (size_t)b * a.slices;
    uint32_t n = 0;
    double s = 0.0;
    for (uint32_t i = 0; i < a.slices; ++i) { n += cnt[i]; s += sum1[i]; }
    const double mean = n ? s / (double)n : 0.0;
    const uint32_t g0 = slice * a.slice_groups;
    const uint32_t g1 = g0 + a.slice_groups < a.groups ? g0 + a.slice_groups : a.groups;
    double q = 0.0;
#pragma unroll 4
    for (uint32_t g = g0 + threadIdx.x; g < g1; g += kThreads) {
        float v[V];
        voxnorm_load<T, VEC>(win, g, a.N, v);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const double d = (double)v[k] - mean;
            q += v[k] != 0.0f ? d * d : 0.0;
        }
    }
    const double q_tot = voxnorm_block_sum(q, tmp);
    if (threadIdx.x == 0) {
        a.sum2[(size_t)b * a.slices + slice] = q_tot;
        if (slice == 0) {
            a.head[(size_t)b * 2] = (double)n;
            a.head[(size_t)b * 2 + 1] = mean;
        }
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void k_voxnorm_write(const VoxnormArgs a) {
    constexpr int V = VoxGroup<T>::V;
    __shared__ float stage[kStageWords];
    const uint32_t b = blockIdx.y, tid = threadIdx.x;
    const T *win = static_cast<const T *>(a.grid) + (size_t)b * a.N;
    float *out = a.out + (size_t)b * a.N;
    double n = 0.0, mean = 0.0, sd = 0.0;
    if (a.normalize) {
        const double *__restrict__ sum2 = a.sum2 + (size_t)b * a.slices;
        n = a.head[(size_t)b * 2];
        mean = a.head[(size_t)b * 2 + 1];
        double q = 0.0;
        for (uint32_t i = 0; i < a.slices; ++i) q += sum2[i];
        sd = n > 0.0 ? sqrt(q / n) : 0.0;
    }
    const bool applied = a.normalize && n > 0.0 && sd > 0.0;
    const double den = 1e-5 + sd;
    if (a.stats && blockIdx.x == 0 && tid == 0) {
        double *st = a.stats + (size_t)b * 4;
        st[0] = n; st[1] = mean; st[2] = sd; st[3] = applied ? 1.0 : 0.0;
    }
    const uint32_t bins = a.bins;
    for (uint32_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const uint32_t px0 = tile * kTilePx;
        const uint32_t npx = a.HW - px0 < (uint32_t)kTilePx ? a.HW - px0 : (uint32_t)kTilePx;
        const uint32_t ne = npx * bins;                      // values of the tile: [px0 * bins, px0 * bins + ne) of the window
        const uint32_t gbase = px0 * bins / V;               // (exact: kTilePx * bins is a multiple of four)
        const uint32_t ng = (ne + V - 1) / V;
        for (uint32_t g = tid; g < ng; g += kThreads) {
            float v[V];
            voxnorm_load<T, VEC>(win, gbase + g, a.N, v);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const uint32_t e = g * V + k;
                float r = v[k];
                if (applied) r = v[k] != 0.0f ? (float)(((double)v[k] - mean) / den) : 0.0f;
                if (e < ne) stage[e + (e >> 5)] = r;
            }
        }
        __syncthreads();
        if (tid < npx) {
            for (uint32_t c = 0; c < bins; ++c) {
                const uint32_t e = tid * bins + c;
                gstore_f32(out + (size_t)c * a.HW + px0 + tid, stage[e + (e >> 5)]);
            }
        }
        __syncthreads();
    }
}

}  // namespace evrep
