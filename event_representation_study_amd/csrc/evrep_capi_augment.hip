// evrep_capi_augment.hip -- the extern "C" surface, part 7: N-ImageNet's event front end and base_augment on the device
// (evrep_augment.hip): argument checks and launches.  No plan, no workspace: the call works on the caller's arrays.
#include "evrep_capi_shared.h"
#include "evrep_augment.hip"

using namespace evrep;
using evrep_host::hip_check;


extern "C" {

size_t evrep_nimg_prepare_scratch_bytes(int32_t B, int64_t total) {
    if (B <= 0 || B > EVREP_NIMG_MAX_B || total < 0) return 0;
    return up256(aug_scratch_bytes(B));
}

int evrep_nimg_prepare(const int32_t *events, const int64_t *offsets, int32_t B, const int64_t *t_base, const evrep_nimg_params *params,
                       double sx, double sy, int32_t img_h, int32_t img_w, uint32_t mode, int32_t *events_out, double *t_out,
                       double *tnorm_out, double *xy_out, int64_t *offsets_out, uint32_t *status_out, void *scratch, void *stream_) {
    if (B < 0 || B > EVREP_NIMG_MAX_B || img_h <= 0 || img_w <= 0 || img_h > EVREP_MAX_DIM || img_w > EVREP_MAX_DIM) return EVREP_EINVAL;
    if (mode & ~(uint32_t)(EVREP_NIMG_TRAIN | EVREP_NIMG_P_UINT8)) return EVREP_EINVAL;
    if (!(sx > 0.0) || !(sy > 0.0) || sx > (double)EVREP_MAX_DIM || sy > (double)EVREP_MAX_DIM) return EVREP_EINVAL;   // (NaN fails too)
    if (bad_ptr(events, 16) || bad_ptr(offsets, 8) || bad_ptr(params, 8) || misaligned(t_base, 8)) return EVREP_EINVAL;
    if (bad_ptr(events_out, 16) || bad_ptr(t_out, 8) || bad_ptr(tnorm_out, 8) || misaligned(xy_out, 16)) return EVREP_EINVAL;
    if (bad_ptr(offsets_out, 8) || bad_ptr(status_out, 4) || bad_ptr(scratch, 16)) return EVREP_EINVAL;
    if (B == 0) return EVREP_OK;
    hipStream_t stream = as_stream(stream_);
    char *sc = static_cast<char *>(scratch);
    uint32_t *slice_cnt = reinterpret_cast<uint32_t *>(sc);
    AugWindow *table = reinterpret_cast<AugWindow *>(sc + aug_off_table());
    uint32_t *kept_cnt = reinterpret_cast<uint32_t *>(sc + aug_off_kept(B));
    if (int rc = hip_check(hipMemsetAsync(table, 0xFF, (size_t)B * sizeof(AugWindow), stream), "hipMemsetAsync(window table)")) return rc;
    if (int rc = hip_check(hipMemsetAsync(kept_cnt, 0, (size_t)B * sizeof(uint32_t), stream), "hipMemsetAsync(kept counts)")) return rc;
    AugArgs a;
    a.ev = reinterpret_cast<const int4 *>(events);
    a.off = offsets;
    a.t_base = t_base;
    a.par = params;
    a.sx = sx;
    a.sy = sy;
    a.res_w = (double)img_w;
    a.res_h = (double)img_h;
    a.B = B;
    a.mode = mode;
    k_nimg_pass<false><<<kAugSlices, kAugThreads, 0, stream>>>(a, slice_cnt, table, kept_cnt, nullptr, nullptr, nullptr, nullptr, nullptr);
    LAUNCH_CHECK("k_nimg_pass(count)");
    k_nimg_scan<<<1, kAugThreads, 0, stream>>>(a, slice_cnt, table, kept_cnt, offsets_out, status_out);
    LAUNCH_CHECK("k_nimg_scan");
    k_nimg_pass<true><<<kAugSlices, kAugThreads, 0, stream>>>(a, slice_cnt, table, kept_cnt, offsets_out, reinterpret_cast<int4 *>(events_out),
                                                            t_out, tnorm_out, reinterpret_cast<double2 *>(xy_out));
    LAUNCH_CHECK("k_nimg_pass(write)");
    return EVREP_OK;
}

}  // extern "C"
