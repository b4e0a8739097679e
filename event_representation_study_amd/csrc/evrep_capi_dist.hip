// evrep_capi_dist.hip -- the extern "C" surface, part 8: N-ImageNet's DiST image and the dense rank of float32 segments on the
// device (evrep_dist.hip): argument checks and launches.  No plan, no workspace: the calls work on the caller's arrays.
#include "evrep_capi_shared.h"
#include "evrep_dist.hip"

using namespace evrep;

static inline bool dist_shape_ok(int32_t B, int32_t H, int32_t W) {
    return B > 0 && B <= EVREP_DIST_MAX_B && H > 0 && W > 0 && H <= EVREP_MAX_DIM && W <= EVREP_MAX_DIM;
}
static inline int64_t dist_tiles_x(int32_t W) { return (W + kTileW - 1) / kTileW; }
static inline int64_t dist_tiles(int32_t H, int32_t W) { return (int64_t)((H + kTileH - 1) / kTileH) * dist_tiles_x(W); }
// scratch of evrep_dist: the 2B clip thresholds, the 2B * H * W discounted times, the pair sort's arrays
static inline size_t dist_off_keys(int32_t B) { return up256((size_t)2 * B * sizeof(uint32_t)); }
static inline size_t dist_off_rank(int32_t B, size_t npx) { return dist_off_keys(B) + up256((size_t)2 * B * npx * sizeof(float)); }

extern "C" {

size_t evrep_dense_rank_scratch_bytes(int32_t S, int64_t total) {
    if (S <= 0 || S > EVREP_RANK_MAX_SEGMENTS || total < 0 || total > EVREP_RANK_MAX_TOTAL) return 0;
    return 4 * rank_array_bytes(total);
}

int evrep_dense_rank_f32(const float *keys, const int64_t *seg_offsets, int32_t S, float *out, int32_t *n_distinct_out, void *scratch,
                         void *stream_) {
    if (S <= 0 || S > EVREP_RANK_MAX_SEGMENTS) return EVREP_EINVAL;
    if (bad_ptr(keys, 4) || bad_ptr(seg_offsets, 8) || bad_ptr(out, 4) || bad_ptr(scratch, 16)) return EVREP_EINVAL;
    if (misaligned(n_distinct_out, 4)) return EVREP_EINVAL;
    RankArgs a;
    a.keys = keys;
    a.offsets = seg_offsets;      // read on the device: the scratch arrays are laid out by seg_offsets[S] there
    a.uniform_len = 0;
    a.S = S;
    a.scratch = static_cast<char *>(scratch);
    a.out = out;
    a.n_distinct = n_distinct_out;
    k_dense_rank<<<S, kDistThreads, 0, as_stream(stream_)>>>(a);
    LAUNCH_CHECK("k_dense_rank");
    return EVREP_OK;
}

size_t evrep_dist_scratch_bytes(int32_t B, int32_t H, int32_t W) {
    if (!dist_shape_ok(B, H, W) || dist_tiles(H, W) * 2 * B > INT32_MAX) return 0;
    const size_t npx = (size_t)H * (size_t)W;
    return dist_off_rank(B, npx) + 4 * rank_array_bytes((int64_t)(2 * (size_t)B * npx));
}

int evrep_dist(const float *prim, int32_t B, int32_t H, int32_t W, double clip_rate, float alpha, float *out, void *scratch, void *stream_) {
    if (!dist_shape_ok(B, H, W) || dist_tiles(H, W) * 2 * B > INT32_MAX) return EVREP_EINVAL;
    if (!(clip_rate >= 0.0) || !(alpha == alpha)) return EVREP_EINVAL;      // (NaN fails)
    if (bad_ptr(prim, 4) || bad_ptr(out, 4) || bad_ptr(scratch, 16)) return EVREP_EINVAL;
    hipStream_t stream = as_stream(stream_);
    const size_t npx = (size_t)H * (size_t)W;
    const int S = 2 * B;
    char *sc = static_cast<char *>(scratch);
    uint32_t *th = reinterpret_cast<uint32_t *>(sc);
    float *keys = reinterpret_cast<float *>(sc + dist_off_keys(B));
    // H * W * CLIP_COUNT_RATE: one float64 multiply; `int64 tensor < Python float` then compares in float32 (torch's type promotion)
    const float limit = (float)((double)((int64_t)H * W) * clip_rate);
    k_dist_clip<<<S, kDistThreads, 0, stream>>>(prim, (int)npx, limit, th);
    LAUNCH_CHECK("k_dist_clip");
    const int tiles = (int)dist_tiles(H, W);
    k_dist_stencil<<<(unsigned)(tiles * S), kStencilThreads, 0, stream>>>(prim, H, W, (int)dist_tiles_x(W), tiles, th, alpha, keys);
    LAUNCH_CHECK("k_dist_stencil");
    RankArgs a;
    a.keys = keys;
    a.offsets = nullptr;
    a.uniform_len = (int64_t)npx;
    a.S = S;
    a.scratch = sc + dist_off_rank(B, npx);
    a.out = out;
    a.n_distinct = nullptr;
    k_dense_rank<<<S, kDistThreads, 0, stream>>>(a);
    LAUNCH_CHECK("k_dense_rank");
    return EVREP_OK;
}

}  // extern "C"
