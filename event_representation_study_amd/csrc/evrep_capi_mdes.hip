// evrep_capi_mdes.hip -- the extern "C" surface, part 2: MixedDensityEventStack / Operations / ERGO-12 (k_mdes).
#define EVREP_TU_MDES 1
#include <cstdlib>
#include "evrep_capi_builders.h"

extern "C" {

int evrep_mdes_sbt_windows(const int32_t *events, const int64_t *offsets, int32_t B, int32_t H, int32_t W, int32_t *bounds,
                           uint32_t *flags, void *stream_) {
    if (bad_ptr(events, 16) || !offsets || !bounds || !flags || B <= 0 || B > 65535 || H <= 0 || W <= 0) return EVREP_EINVAL;
    k_mdes_sbt_windows<<<B, 1024, 0, as_stream(stream_)>>>(reinterpret_cast<const int4 *>(events), offsets, H, W, bounds, flags);
    LAUNCH_CHECK("k_mdes_sbt_windows");
    return EVREP_OK;
}

int evrep_mdes(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace, int32_t C,
               const int32_t *window, const int32_t *func, const int32_t *agg, double scale, int32_t out_dtype,
               void *out, void *stream_) {
    return evrep_mdes_ex(plan, events, offsets, workspace, C, window, func, agg, scale, out_dtype, out, nullptr, nullptr, stream_);
}

int evrep_mdes_ex(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace, int32_t C,
                  const int32_t *window, const int32_t *func, const int32_t *agg, double scale, int32_t out_dtype,
                  void *out, const int32_t *bounds, const uint32_t *flags, void *stream_) {
    int rc = check_common(plan, events, offsets, workspace);
    if (rc) return rc;
    if (C <= 0 || C > EVREP_MAX_CHANNELS || !window || !func || !agg || !out) return EVREP_EINVAL;
    if (!is_float_dtype(out_dtype)) return EVREP_EINVAL;
    if ((bounds == nullptr) != (flags == nullptr)) return EVREP_EINVAL;
    hipStream_t stream = as_stream(stream_);
    MdesParams P;
    memset(&P, 0, sizeof(P));
    P.C = C;
    P.bounds = bounds;
    P.wflags = flags;
    for (int c = 0; c < C; ++c) { P.win[c] = window[c]; P.func[c] = func[c]; P.agg[c] = agg[c]; }
    // the ERGO-12 triples get the kernel instance with compile-time descriptors
    bool ergo = C == Ergo12Table::kC && bounds == nullptr;
    for (int c = 0; ergo && c < C; ++c)
        ergo = window[c] == Ergo12Table::kWin[c] && func[c] == Ergo12Table::kFunc[c] && agg[c] == Ergo12Table::kAgg[c];
    // after the key-sorted pass: ERGO-12 as a stream (k_mdes_stream) -- one launch, every unit, no hot list -- where it wins
    if (ergo && stream_allowed(plan, EVREP_PLAN_X_MDES_ORDERED) &&
        ((plan->flags & EVREP_PLAN_X_MDES_STREAM) || records_per_unit(plan) > (out_dtype == EVREP_F32 ? kErgoStreamMinPerUnitF32 : kErgoStreamMinPerUnitF64))) {
        const UnitCfg us = stream_cfg(plan, unit_cfg(plan, (size_t)C * (out_dtype == EVREP_F64 ? 8 : 4)));
        constexpr int kRB = 4;
        auto launch = [&](auto t) {
            using T = typename decltype(t)::type;
            k_mdes_stream<T, kRB><<<unit_grid(plan, us), kWave, mdes_stream_lds_bytes(kChunkPx, sizeof(T), kRB), stream>>>(
                bin_view(plan, events, workspace, true), offsets, plan->H, plan->W, plan->nchunk, us, scale, static_cast<T *>(out));
        };
        if (out_dtype == EVREP_F64) launch(Type<double>()); else launch(Type<float>());
        LAUNCH_CHECK("k_mdes_stream");
        return EVREP_OK;
    }
    if (int rc3 = ensure_pixel_stream(plan, events, offsets, workspace, stream)) return rc3;
    UnitCfg uc = unit_cfg(plan, (size_t)C * (out_dtype == EVREP_F64 ? 8 : 4));
    if ((plan->flags & EVREP_PLAN_X_SPAN2) && plan->nchunk >= 2) { uc.span = 2; uc.stage = 128; unit_cfg_geometry(uc, plan); }
    const int seg = (uc.span + uc.merge) * kChunkPx;
    const bool pace_auto = plan->pacing < 0 && out_dtype == EVREP_F64 && C * 8 >= 64;   // the store-bound instances
    auto launch = [&](auto t, auto desc) {
        using T = typename decltype(t)::type;
        using DESC = typename decltype(desc)::type;
        constexpr bool kErgo = MdesIsErgo12<DESC>::value;
        const size_t lds = chunk_lds_bytes(C, sizeof(T), seg, uc.stage, uc.partpx);
        // the float64 ERGO-12 instance defers nothing (its split path, mdes_unit): no hot launch behind it; the float32 one
        // hands hot units to its hot launch whole (Split, IN_HOT): a stage of kHotSplitStage records there -- and, r06, units of
        // >= kErgoCoopMin records to a cooperative launch of sixteen waves per unit (k_mdes_coop; kXfCoopErgo12)
        const bool hot_launch = ks_pass(plan) && !(kErgo && sizeof(T) == 8);
        const bool coop = hot_launch && kErgo && sizeof(T) == 4 && !(plan->flags & EVREP_PLAN_X_MDES_NO_COOP);
        if (coop) uc.xflags |= kXfCoopErgo12;
        if (pace_auto) uc.hold = auto_hold(plan, reinterpret_cast<const void *>(&k_mdes<T, DESC>), lds, uc.span, (size_t)C * sizeof(T), uc.merge);
        k_mdes<T, DESC><<<unit_grid(plan, uc), kWave, lds, stream>>>(bin_view(plan, events, workspace), offsets, P, plan->H, plan->W,
                                                                   plan->nchunk, uc, scale, static_cast<T *>(out));
        UnitCfg hc = hot_cfg(uc);
        if (kErgo) hc.stage = hot_sweep_stage((size_t)seg * 7 * 4, 4096, (size_t)uc.partpx * C * sizeof(T));
        if (coop) {
            if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mdes_coop), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024) != hipSuccess) {
                (void)hipGetLastError();
                return EVREP_EHIP;
            }
            k_mdes_coop<<<kMcGrid, kMcThreads, mdes_coop_lds_bytes(seg), stream>>>(bin_view(plan, events, workspace), offsets, plan->H, plan->W, plan->nchunk, uc, scale,
                                                                                  reinterpret_cast<float *>(out));
        }
        if (hot_launch) k_mdes<T, DESC, true><<<kHotGrid, kWave, chunk_lds_bytes(C, sizeof(T), seg, hc.stage, uc.partpx), stream>>>(
            bin_view(plan, events, workspace), offsets, P, plan->H, plan->W, plan->nchunk, hc, scale, static_cast<T *>(out));
        return EVREP_OK;
    };
    auto launch_for = [&](auto t) {
        if (ergo) return launch(t, Type<StaticDesc<Ergo12Table>>());
        if (C <= 4) return launch(t, Type<RuntimeDesc<4>>());
        if (C <= 8) return launch(t, Type<RuntimeDesc<8>>());
        if (C <= 12) return launch(t, Type<RuntimeDesc<12>>());
        return launch(t, Type<RuntimeDesc<16>>());
    };
    if (int rc4 = out_dtype == EVREP_F64 ? launch_for(Type<double>()) : launch_for(Type<float>())) return rc4;
    LAUNCH_CHECK("k_mdes");
    return EVREP_OK;
}

int evrep_optimized(const evrep_plan *plan, const int32_t *events, const int64_t *offsets, void *workspace,
                    double scale, int32_t out_dtype, void *out, void *stream) {
    int32_t win[12], func[12], agg[12];
    for (int c = 0; c < 12; ++c) { win[c] = Ergo12Table::kWin[c]; func[c] = Ergo12Table::kFunc[c]; agg[c] = Ergo12Table::kAgg[c]; }
    return evrep_mdes(plan, events, offsets, workspace, 12, win, func, agg, scale, out_dtype, out, stream);
}

}  // extern "C"
