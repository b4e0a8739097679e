// evrep_capi_study.hip -- the extern "C" surface, part 13: the rows of the study's representations from an N-ImageNet front-end
// batch (evrep_study.hip): argument checks, one memset and two launches.  No plan, no workspace: the call works on the caller's
// arrays.
#include "evrep_capi_shared.h"
#include "evrep_study.hip"

using namespace evrep;
using evrep_host::hip_check;


extern "C" {

size_t evrep_nimg_study_rows_scratch_bytes(int32_t B, int64_t total) {
    if (B <= 0 || B > EVREP_NIMG_MAX_B || total < 0) return 0;
    return up256(study_scratch_bytes(B));
}

int evrep_nimg_study_rows(const int32_t *rows, const double *t, const double *xy, const int64_t *offsets, int32_t B, int32_t H,
                          int32_t W, uint32_t want, int32_t *rows_mdes, int32_t *rows_stack, int32_t *rows_tore,
                          double *sample_times, uint32_t *status, void *scratch, void *stream_) {
    if (B < 0 || B > EVREP_NIMG_MAX_B || H <= 0 || W <= 0 || H > EVREP_MAX_DIM || W > EVREP_MAX_DIM) return EVREP_EINVAL;
    if (want == 0u || (want & ~(uint32_t)(EVREP_STUDY_MDES | EVREP_STUDY_STACK | EVREP_STUDY_TORE))) return EVREP_EINVAL;
    if (bad_ptr(rows, 16) || bad_ptr(t, 8) || bad_ptr(offsets, 8) || bad_ptr(status, 4) || bad_ptr(scratch, 16)) return EVREP_EINVAL;
    if ((want & EVREP_STUDY_MDES) && bad_ptr(rows_mdes, 16)) return EVREP_EINVAL;
    if ((want & EVREP_STUDY_STACK) && bad_ptr(rows_stack, 16)) return EVREP_EINVAL;
    if ((want & EVREP_STUDY_TORE) && (bad_ptr(rows_tore, 16) || bad_ptr(xy, 16) || bad_ptr(sample_times, 8))) return EVREP_EINVAL;
    if (B == 0) return EVREP_OK;
    hipStream_t stream = as_stream(stream_);
    StudyWindow *win = static_cast<StudyWindow *>(scratch);
    if (int rc = hip_check(hipMemsetAsync(win, 0xFF, study_scratch_bytes(B), stream), "hipMemsetAsync(study windows)")) return rc;
    StudyArgs a;
    a.rows = reinterpret_cast<const int4 *>(rows);
    a.t = t;
    a.xy = reinterpret_cast<const double2 *>(xy);
    a.off = offsets;
    a.B = B;
    a.want = want;
    k_study_reduce<<<kStudyBlocks, kStudyThreads, 0, stream>>>(a, win);
    LAUNCH_CHECK("k_study_reduce");
    // an output that is not wanted is not written, whatever the caller passed for it
    k_study_write<<<kStudyBlocks, kStudyThreads, 0, stream>>>(a, win, (want & EVREP_STUDY_MDES) ? reinterpret_cast<int4 *>(rows_mdes) : nullptr,
                                                            (want & EVREP_STUDY_STACK) ? reinterpret_cast<int4 *>(rows_stack) : nullptr,
                                                            (want & EVREP_STUDY_TORE) ? reinterpret_cast<int4 *>(rows_tore) : nullptr,
                                                            (want & EVREP_STUDY_TORE) ? sample_times : nullptr, status);
    LAUNCH_CHECK("k_study_write");
    return EVREP_OK;
}

}  // extern "C"
