// evrep_capi_sort.hip -- the extern "C" surface, part 9: N-ImageNet's sorted timestamp image on the device (evrep_sort.hip):
// argument checks and launches.  No plan, no workspace: the calls work on the caller's arrays.
#include "evrep_capi_shared.h"
#include "evrep_sort.hip"

using namespace evrep;
using evrep_host::hip_check;

static inline bool sort_shape_ok(int32_t B, int32_t H, int32_t W, int32_t K) {
    return B > 0 && B <= EVREP_SORT_MAX_B && H > 0 && W > 0 && H <= EVREP_MAX_DIM && W <= EVREP_MAX_DIM && (K == 1 || K == 2);
}

extern "C" {

size_t evrep_time_index_scratch_bytes(int32_t B, int64_t total) {
    if (B <= 0 || B > EVREP_SORT_MAX_B || total < 0 || total > (int64_t)UINT32_MAX) return 0;
    return up256(ti_scratch_bytes(B));
}

int evrep_time_index(const double *t, const int64_t *offsets, int32_t B, int32_t mode, double *out, uint32_t *status_out, void *scratch,
                     void *stream_) {
    if (B < 0 || B > EVREP_SORT_MAX_B || (mode != EVREP_TIME_INDEX_RAW && mode != EVREP_TIME_INDEX_RANK)) return EVREP_EINVAL;
    if (bad_ptr(t, 8) || bad_ptr(offsets, 8) || bad_ptr(out, 8) || bad_ptr(status_out, 4) || bad_ptr(scratch, 16)) return EVREP_EINVAL;
    if (B == 0) return EVREP_OK;
    hipStream_t stream = as_stream(stream_);
    char *sc = static_cast<char *>(scratch);
    uint32_t *slice_cnt = reinterpret_cast<uint32_t *>(sc);
    uint32_t *win_start = reinterpret_cast<uint32_t *>(sc + ti_off_start());
    uint32_t *win_slice = reinterpret_cast<uint32_t *>(sc + ti_off_slice(B));
    if (int rc = hip_check(hipMemsetAsync(status_out, 0, (size_t)B * sizeof(uint32_t), stream), "hipMemsetAsync(status)")) return rc;
    TiArgs a;
    a.t = t;
    a.off = offsets;
    a.B = B;
    a.mode = mode;
    k_ti_pass<false><<<kTiSlices, kTiThreads, 0, stream>>>(a, slice_cnt, win_start, win_slice, nullptr, status_out);
    LAUNCH_CHECK("k_ti_pass(count)");
    k_ti_scan<<<1, kTiThreads, 0, stream>>>(a, slice_cnt, win_start, win_slice, status_out);
    LAUNCH_CHECK("k_ti_scan");
    k_ti_pass<true><<<kTiSlices, kTiThreads, 0, stream>>>(a, slice_cnt, win_start, win_slice, out, status_out);
    LAUNCH_CHECK("k_ti_pass(write)");
    return EVREP_OK;
}

size_t evrep_sort_image_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t K) {
    if (!sort_shape_ok(B, H, W, K)) return 0;
    return 4 * rank_array_bytes((int64_t)B * K * H * W);
}

int evrep_sort_image(const float *prim, int32_t B, int32_t H, int32_t W, int32_t K, uint32_t flags, const int32_t *quantize, int32_t nq,
                     float *out, uint32_t *status, void *scratch, void *stream_) {
    if (!sort_shape_ok(B, H, W, K) || (flags & ~(uint32_t)(EVREP_SORT_STRICT | EVREP_SORT_USE_IMAGE))) return EVREP_EINVAL;
    if (nq < 0 || nq > EVREP_SORT_MAX_Q || (nq > 0 && !quantize)) return EVREP_EINVAL;
    if (bad_ptr(prim, 4) || bad_ptr(out, 4) || bad_ptr(status, 4) || bad_ptr(scratch, 16)) return EVREP_EINVAL;
    SortImageArgs a;
    for (int c = 0; c < nq; ++c) {
        if (quantize[c] <= 0) return EVREP_EINVAL;
        a.q[c] = (float)quantize[c];                      // torch multiplies a float32 tensor by a Python int as a float32 scalar
    }
    for (int c = nq; c < EVREP_SORT_MAX_Q; ++c) a.q[c] = 1.0f;
    a.prim = prim;
    a.out = out;
    a.status = status;
    a.scratch = static_cast<char *>(scratch);
    a.B = B;
    a.K = K;
    a.npx = H * W;
    a.strict = (flags & EVREP_SORT_STRICT) ? 1 : 0;
    a.use_image = (flags & EVREP_SORT_USE_IMAGE) ? 1 : 0;
    a.nq = nq;
    k_sort_image<<<(unsigned)(B * K), kDistThreads, 0, as_stream(stream_)>>>(a);
    LAUNCH_CHECK("k_sort_image");
    return EVREP_OK;
}

}  // extern "C"
