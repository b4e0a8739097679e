// evrep_capi_voxnorm.hip -- the extern "C" surface, part 11: ev-licious' normalised, channel-first voxel grid batch
// (evrep_voxnorm.hip): argument checks and three launches.  No plan, no workspace: the call works on the caller's arrays.
#include "evrep_capi_shared.h"
#include "evrep_voxnorm.hip"

using namespace evrep;

// values of a window, or 0 for sizes the entry points refuse
static inline uint32_t voxnorm_window(int32_t B, int32_t H, int32_t W, int32_t bins) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || bins < 1 || bins > EVREP_MAX_CHANNELS) return 0;   // windows ride gridDim.y
    const int64_t hw = (int64_t)H * W;
    if (hw >= ((int64_t)1 << 31) || hw * bins >= ((int64_t)1 << 31)) return 0;
    return (uint32_t)(hw * bins);
}

// the slices of a window for groups of V values
static inline void voxnorm_geometry(uint32_t N, uint32_t V, VoxnormArgs &a) {
    a.N = N;
    a.groups = (N + V - 1) / V;
    a.slice_groups = voxnorm_slice_groups(a.groups);
    a.slices = (a.groups + a.slice_groups - 1) / a.slice_groups;
}

// scratch: sum1, sum2 [B][slices] double, cnt [B][slices] uint32, each sized for kMaxSlices slices of double, then head [B][2]
// double; into `a`.  Returns the region's bytes
static inline size_t voxnorm_carve(void *scratch, int32_t B, VoxnormArgs &a) {
    Carver c(scratch);
    const size_t part = (size_t)B * kMaxSlices * sizeof(double);
    a.sum1 = c.take<double>(part);
    a.sum2 = c.take<double>(part);
    a.cnt = c.take<uint32_t>(part);
    a.head = c.take<double>((size_t)B * 2 * sizeof(double));
    return c.off;
}

template <typename T, bool VEC>
static int voxnorm_launch(const VoxnormArgs &a, int32_t B, hipStream_t stream) {
    if (a.normalize) {
        const dim3 grid(a.slices, (unsigned)B);
        k_voxnorm_sum<T, VEC><<<grid, kThreads, 0, stream>>>(a);
        LAUNCH_CHECK("k_voxnorm_sum");
        k_voxnorm_sqdev<T, VEC><<<grid, kThreads, 0, stream>>>(a);
        LAUNCH_CHECK("k_voxnorm_sqdev");
    }
    const dim3 grid(a.tiles < (uint32_t)kWriteBlocks ? a.tiles : (uint32_t)kWriteBlocks, (unsigned)B);
    k_voxnorm_write<T, VEC><<<grid, kThreads, 0, stream>>>(a);
    LAUNCH_CHECK("k_voxnorm_write");
    return EVREP_OK;
}

extern "C" {

size_t evrep_voxel_normalize_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t bins) {
    if (!voxnorm_window(B, H, W, bins)) return 0;
    VoxnormArgs a;
    return voxnorm_carve(nullptr, B, a);
}

int evrep_voxel_normalize(const void *grid, int32_t grid_dtype, int32_t B, int32_t H, int32_t W, int32_t bins, uint32_t flags,
                          float *out, double *stats_out, void *scratch, void *stream_) {
    if (!is_float_dtype(grid_dtype)) return EVREP_EINVAL;
    if (flags & ~EVREP_VOXNORM_NORMALIZE) return EVREP_EINVAL;
    const uint32_t N = voxnorm_window(B, H, W, bins);
    if (!N) return EVREP_EINVAL;
    const bool normalize = (flags & EVREP_VOXNORM_NORMALIZE) != 0u;
    if (bad_ptr(grid, 16) || bad_ptr(out, 16)) return EVREP_EINVAL;
    if (normalize ? bad_ptr(scratch, 16) : stats_out != nullptr) return EVREP_EINVAL;   // statistics come with the normalisation
    if (misaligned(stats_out, 16)) return EVREP_EINVAL;
    const uint32_t V = grid_dtype == EVREP_F64 ? 2u : 4u;
    VoxnormArgs a;
    memset(&a, 0, sizeof(a));
    voxnorm_geometry(N, V, a);
    a.grid = grid; a.out = out; a.stats = stats_out;
    if (normalize) voxnorm_carve(scratch, B, a);
    a.HW = (uint32_t)((int64_t)H * W);
    a.bins = (uint32_t)bins;
    a.tiles = (a.HW + kTilePx - 1) / kTilePx;
    a.normalize = normalize ? 1u : 0u;
    // one 16-byte load per group where every window starts on a 16-byte boundary; the grouping, and with it every sum, is the same
    const bool vec = N % V == 0;
    hipStream_t stream = as_stream(stream_);
    if (grid_dtype == EVREP_F64) return vec ? voxnorm_launch<double, true>(a, B, stream) : voxnorm_launch<double, false>(a, B, stream);
    return vec ? voxnorm_launch<float, true>(a, B, stream) : voxnorm_launch<float, false>(a, B, stream);
}

}  // extern "C"
