// evrep_capi_filters.hip -- the extern "C" surface, part 5: the ev-licious event filters (evrep_filters.hip): argument checks
// and launches.  The filters read the pixel-sorted stream; after the key-sorted pass (plan->reserved == 2), which leaves block
// runs only, the per-key column sort of evrep_capi.hip is run in front of them, as it is for every other consumer of that stream.
#include "evrep_capi_shared.h"
#include "evrep_filters.hip"

using namespace evrep;
using evrep_host::hip_check;

// the window time bases, HOST -> the workspace slot that evrep_time_surface's cuts use between its own launches (every
// time-surface call forms its cuts anew): B * 8 of its B * kTsCutsBytes bytes.  NULL stays NULL (base 0).
static int stage_t_base(const evrep_plan *plan, void *workspace, const int64_t *t_base, hipStream_t stream, const int64_t **dev) {
    *dev = nullptr;
    if (!t_base) return EVREP_OK;
    int64_t *slot = WS(int64_t, off_cuts);
    static_assert(kTsCutsBytes >= sizeof(int64_t), "one time base per window fits the cuts slot");
    *dev = slot;
    return hip_check(hipMemcpyAsync(slot, t_base, (size_t)plan->B * sizeof(int64_t), hipMemcpyHostToDevice, stream),
                     "hipMemcpyAsync(t_base)");
}

static int pixel_stream(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace, hipStream_t stream) {
    if (plan->reserved != 2) return EVREP_OK;
    return evrep_host::column_sort_keys(plan, events, offsets, workspace, stream);
}

static inline dim3 event_grid(const evrep_plan *plan) {
    const int64_t n = plan->max_events_per_window > 0 ? plan->max_events_per_window : 1;
    return dim3((unsigned)((n + kFiltThreads - 1) / kFiltThreads), (unsigned)plan->B);
}

extern "C" {

int evrep_filter_pixel_fsm(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace, int32_t kind,
                           double param, const int64_t *t_base, void *state, uint8_t *keep, void *stream_) {
    int rc = check_common(plan, events, offsets, workspace);
    if (rc) return rc;
    if (kind != EVREP_FILTER_REFRACTORY && kind != EVREP_FILTER_CONTRAST && kind != EVREP_FILTER_CHANGE_MAP) return EVREP_EINVAL;
    if (!(param > 0.0) || bad_ptr(state, kind == EVREP_FILTER_REFRACTORY ? 8 : 4)) return EVREP_EINVAL;
    if (plan->total_events > 0 && !keep) return EVREP_EINVAL;
    if (plan->total_events == 0) return EVREP_OK;
    hipStream_t stream = as_stream(stream_);
    if (int rc2 = pixel_stream(plan, events, offsets, workspace, stream)) return rc2;
    const int64_t *tb = nullptr;
    if (kind == EVREP_FILTER_REFRACTORY) if (int rc2 = stage_t_base(plan, workspace, t_base, stream, &tb)) return rc2;
    if (int rc2 = hip_check(hipMemsetAsync(keep, 0, (size_t)plan->total_events, stream), "hipMemsetAsync(keep)")) return rc2;
    const Rec *sorted = CWS(Rec, off_sorted2);
    const uint32_t *co = CWS(uint32_t, off_chunkoff);
    const dim3 grid = event_grid(plan);
#define FSM_LAUNCH(F, MEMBER)                                                                                                      \
    do {                                                                                                                       \
        F f_;                                                                                                                  \
        MEMBER = param;                                                                                                          \
        k_filter_pixel_fsm<F><<<grid, kFiltThreads, 0, stream>>>(sorted, co, offsets, tb, reinterpret_cast<const int4 *>(events), \
                                                               CWS(WindowMeta, off_meta), plan->H, plan->W, plan->nchunk, f_,   \
                                                               static_cast<F::S *>(state), keep);                             \
    } while (0)
    if (kind == EVREP_FILTER_REFRACTORY) FSM_LAUNCH(FsmRefractory, f_.period);
    else if (kind == EVREP_FILTER_CONTRAST) FSM_LAUNCH(FsmContrast, f_.factor);
    else FSM_LAUNCH(FsmChangeMap, f_.cells);
#undef FSM_LAUNCH
    LAUNCH_CHECK("k_filter_pixel_fsm");
    return EVREP_OK;
}

int evrep_filter_background(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace, double depth,
                            int32_t radius, const int64_t *t_base, double *state, uint8_t *keep, void *stream_) {
    int rc = check_common(plan, events, offsets, workspace);
    if (rc) return rc;
    if (!(depth > 0.0) || radius < 1 || radius > EVREP_FILTER_MAX_RADIUS || bad_ptr(state, 8)) return EVREP_EINVAL;
    if (plan->total_events > 0 && !keep) return EVREP_EINVAL;
    if (plan->total_events == 0) return EVREP_OK;
    hipStream_t stream = as_stream(stream_);
    if (int rc2 = pixel_stream(plan, events, offsets, workspace, stream)) return rc2;
    const int64_t *tb = nullptr;
    if (int rc2 = stage_t_base(plan, workspace, t_base, stream, &tb)) return rc2;
    const Rec *sorted = CWS(Rec, off_sorted2);
    const uint32_t *co = CWS(uint32_t, off_chunkoff);
    k_filter_background<<<event_grid(plan), kFiltThreads, 0, stream>>>(reinterpret_cast<const int4 *>(events), sorted, co, offsets, tb,
                                                                     CWS(WindowMeta, off_meta), plan->H, plan->W, plan->nchunk, depth, radius,
                                                                     state, keep);
    LAUNCH_CHECK("k_filter_background");
    const dim3 pgrid((unsigned)(((size_t)plan->H * plan->W + kFiltThreads - 1) / kFiltThreads), (unsigned)plan->B);
    k_filter_background_state<<<pgrid, kFiltThreads, 0, stream>>>(sorted, co, offsets, tb, reinterpret_cast<const int4 *>(events),
                                                                CWS(WindowMeta, off_meta), plan->H, plan->W, plan->nchunk, radius, state);
    LAUNCH_CHECK("k_filter_background_state");
    return EVREP_OK;
}

int evrep_filter_mask_gather(const int32_t *events, const int64_t *offsets, int32_t B, int32_t H, int32_t W,
                             int64_t max_events_per_window, const uint8_t *mask, uint8_t *keep, void *stream_) {
    if (!offsets || !mask || !keep || B <= 0 || B > 65535 || H <= 0 || W <= 0 || H > EVREP_MAX_DIM || W > EVREP_MAX_DIM) return EVREP_EINVAL;
    if (max_events_per_window < 0 || max_events_per_window >= (int64_t)1 << 31) return EVREP_EINVAL;
    if (max_events_per_window > 0 && bad_ptr(events, 16)) return EVREP_EINVAL;
    if (max_events_per_window == 0) return EVREP_OK;
    const dim3 grid((unsigned)((max_events_per_window + kFiltThreads - 1) / kFiltThreads), (unsigned)B);
    k_filter_mask_gather<<<grid, kFiltThreads, 0, as_stream(stream_)>>>(reinterpret_cast<const int4 *>(events), offsets, H, W, mask, keep);
    LAUNCH_CHECK("k_filter_mask_gather");
    return EVREP_OK;
}

int evrep_filter_cell_map(const int32_t *events, int64_t total, int32_t H, int32_t W, int32_t fy, int32_t fx, int32_t *events_out,
                          void *stream_) {
    if (total < 0 || total >= (int64_t)1 << 31 || H <= 0 || W <= 0 || H > EVREP_MAX_DIM || W > EVREP_MAX_DIM) return EVREP_EINVAL;
    if (fx < 1 || fy < 1 || fx > W || fy > H) return EVREP_EINVAL;
    if (total > 0 && (bad_ptr(events, 16) || bad_ptr(events_out, 16))) return EVREP_EINVAL;
    if (total == 0) return EVREP_OK;
    const uint32_t mx = fx == 1 ? 0u : (uint32_t)(((uint64_t)1 << 32) / (uint32_t)fx + 1u);
    const uint32_t my = fy == 1 ? 0u : (uint32_t)(((uint64_t)1 << 32) / (uint32_t)fy + 1u);
    k_filter_cell_map<<<(unsigned)((total + kFiltThreads - 1) / kFiltThreads), kFiltThreads, 0, as_stream(stream_)>>>(
        reinterpret_cast<const int4 *>(events), total, H, W, mx, my, reinterpret_cast<int4 *>(events_out));
    LAUNCH_CHECK("k_filter_cell_map");
    return EVREP_OK;
}

size_t evrep_filter_compact_scratch_bytes(int32_t B, int64_t total) {
    if (B <= 0 || total < 0) return 0;
    return up256(filter_compact_scratch_bytes());
}

int evrep_filter_compact(const int32_t *events, const int64_t *offsets, int32_t B, const uint8_t *keep, int32_t *events_out,
                         int64_t *offsets_out, void *scratch, void *stream_) {
    if (!offsets || !keep || B <= 0 || B > 65535) return EVREP_EINVAL;   // (a batch without events still owns one-row allocations)
    if (bad_ptr(events, 16) || bad_ptr(events_out, 16) || bad_ptr(offsets_out, 8) || bad_ptr(scratch, 16)) return EVREP_EINVAL;
    hipStream_t stream = as_stream(stream_);
    const int4 *ev = reinterpret_cast<const int4 *>(events);
    uint32_t *sc = static_cast<uint32_t *>(scratch);
    k_filter_compact<false><<<kCompactSlices, kCompactThreads, 0, stream>>>(ev, offsets, B, keep, sc, nullptr);
    LAUNCH_CHECK("k_filter_compact(count)");
    k_filter_compact_scan<<<1, kCompactThreads, 0, stream>>>(sc);
    LAUNCH_CHECK("k_filter_compact_scan");
    k_filter_compact<true><<<kCompactSlices, kCompactThreads, 0, stream>>>(ev, offsets, B, keep, sc, reinterpret_cast<int4 *>(events_out));
    LAUNCH_CHECK("k_filter_compact(write)");
    k_filter_compact_offsets<<<B + 1, kWave, 0, stream>>>(offsets, B, keep, sc, offsets_out);
    LAUNCH_CHECK("k_filter_compact_offsets");
    return EVREP_OK;
}

}  // extern "C"
