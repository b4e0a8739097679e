// evrep_capi_windows.hip -- the extern "C" surface, part 6: windows cut from a device-resident recording
// (evrep_windows.hip): argument checks and launches.  No plan, no workspace: both calls work on the caller's arrays.
#include "evrep_capi_shared.h"
#include "evrep_windows.hip"

using namespace evrep;
using evrep_host::hip_check;


extern "C" {

int evrep_time_to_index(const int64_t *t, int64_t n, const int64_t *queries, int64_t nq, int64_t *out_idx, void *stream_) {
    if (n < 0 || nq < 0 || nq > EVREP_WINDOWS_MAX_QUERIES) return EVREP_EINVAL;
    if (misaligned(t, 8) || (n > 0 && !t)) return EVREP_EINVAL;
    if (misaligned(queries, 8) || misaligned(out_idx, 8) || (nq > 0 && (!queries || !out_idx))) return EVREP_EINVAL;
    if (nq == 0) return EVREP_OK;
    const unsigned grid = (unsigned)((nq + kWinThreads / kWave - 1) / (kWinThreads / kWave));
    k_time_to_index<<<grid, kWinThreads, 0, as_stream(stream_)>>>(t, n, queries, nq, out_idx);
    LAUNCH_CHECK("k_time_to_index");
    return EVREP_OK;
}

int evrep_windows_gather(const uint16_t *x, const uint16_t *y, const int64_t *t, const int8_t *p, int64_t n, const int64_t *i0,
                         const int64_t *i1, const int64_t *dst_offsets, int32_t B, int32_t rebase_mode, const int64_t *base_in,
                         int32_t *events_out, int64_t *base_out, uint32_t *status_out, void *stream_) {
    if (n < 0 || B < 0 || B > EVREP_WINDOWS_MAX_B) return EVREP_EINVAL;
    if (rebase_mode != EVREP_REBASE_NONE && rebase_mode != EVREP_REBASE_FIRST && rebase_mode != EVREP_REBASE_GIVEN) return EVREP_EINVAL;
    if (misaligned(x, 2) || misaligned(y, 2) || misaligned(t, 8) || (n > 0 && (!x || !y || !t || !p))) return EVREP_EINVAL;
    if (bad_ptr(i0, 8) || bad_ptr(i1, 8) || bad_ptr(dst_offsets, 8)) return EVREP_EINVAL;
    if (bad_ptr(events_out, 16) || bad_ptr(base_out, 8) || bad_ptr(status_out, 4)) return EVREP_EINVAL;
    if (misaligned(base_in, 8) || (rebase_mode == EVREP_REBASE_GIVEN && !base_in)) return EVREP_EINVAL;
    if (B == 0) return EVREP_OK;
    hipStream_t stream = as_stream(stream_);
    if (int rc = hip_check(hipMemsetAsync(status_out, 0, (size_t)B * sizeof(uint32_t), stream), "hipMemsetAsync(status_out)")) return rc;
    k_windows_gather<<<kGatherGrid, kWinThreads, 0, stream>>>(x, y, t, p, n, i0, i1, dst_offsets, B, rebase_mode, base_in,
                                                             reinterpret_cast<int4 *>(events_out), base_out, status_out);
    LAUNCH_CHECK("k_windows_gather");
    return EVREP_OK;
}

}  // extern "C"
