// evrep_capi_detin.hip -- the extern "C" surface, part 10: the detector's input batch (evrep_detin.hip): argument checks and
// the one launch.  No plan, no workspace, no allocation, no wait for the device.
#include "evrep_capi_shared.h"
#include "evrep_detin.hip"

using namespace evrep;
using evrep_host::hip_check;

static inline bool bad_ptr(const void *p, uintptr_t a) { return !p || (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

template <typename T>
static int detin_launch(const DetinArgs<double> &d, const void *rep, int32_t B, hipStream_t stream) {
    DetinArgs<T> a;
    a.src = static_cast<const T *>(rep);
    a.ystart = d.ystart; a.ycount = d.ycount; a.xstart = d.xstart; a.xcount = d.xcount; a.ywt = d.ywt; a.xwt = d.xwt;
    a.pad = d.pad; a.flags = d.flags; a.warp = d.warp; a.out = d.out;
    a.H = d.H; a.W = d.W; a.C = d.C; a.nh = d.nh; a.nw = d.nw; a.Tt = d.Tt; a.S = d.S; a.top = d.top; a.left = d.left;
    a.scale = d.scale;
    const int P = kThreads / ((d.C + kDetinGroup - 1) / kDetinGroup);   // pixels of a workgroup (evrep_detin.hip)
    const dim3 grid((unsigned)(((size_t)d.S * d.S + P - 1) / P), (unsigned)B);
    k_detector_input<T><<<grid, kThreads, 0, stream>>>(a);
    LAUNCH_CHECK("k_detector_input");
    return EVREP_OK;
}

extern "C" {

int evrep_detector_input(const void *rep, int32_t rep_dtype, int32_t B, int32_t H, int32_t W, int32_t C, int32_t nh, int32_t nw,
                         int32_t T, const int32_t *ystart, const int32_t *ycount, const double *ywt, const int32_t *xstart,
                         const int32_t *xcount, const double *xwt, int32_t S, int32_t top, int32_t left, const double *pad,
                         const uint32_t *flags, const int32_t *warp, float scale, float *out, void *stream_) {
    if (rep_dtype != EVREP_F64 && rep_dtype != EVREP_F32) return EVREP_EINVAL;
    if (B <= 0 || B > 65535 || C < 1 || C > EVREP_MAX_CHANNELS) return EVREP_EINVAL;
    if (H < 1 || W < 1 || H > EVREP_MAX_DIM || W > EVREP_MAX_DIM || S < 1 || S > EVREP_MAX_DIM) return EVREP_EINVAL;
    if (nh < 1 || nw < 1 || top < 0 || left < 0 || nh > S - top || nw > S - left || T < 1 || T > EVREP_MAX_DIM) return EVREP_EINVAL;
    if (!(scale == scale)) return EVREP_EINVAL;   // NaN
    if (bad_ptr(rep, rep_dtype == EVREP_F64 ? 8 : 4) || bad_ptr(out, 4) || bad_ptr(pad, 8)) return EVREP_EINVAL;
    if (bad_ptr(ystart, 4) || bad_ptr(ycount, 4) || bad_ptr(ywt, 8) || bad_ptr(xstart, 4) || bad_ptr(xcount, 4) || bad_ptr(xwt, 8))
        return EVREP_EINVAL;
    if (flags ? (bad_ptr(flags, 4) || bad_ptr(warp, 4)) : warp != nullptr) return EVREP_EINVAL;   // the two come together
    DetinArgs<double> d;
    memset(&d, 0, sizeof(d));
    d.ystart = ystart; d.ycount = ycount; d.xstart = xstart; d.xcount = xcount; d.ywt = ywt; d.xwt = xwt;
    d.pad = pad; d.flags = flags; d.warp = warp; d.out = out;
    d.H = H; d.W = W; d.C = C; d.nh = nh; d.nw = nw; d.Tt = T; d.S = S; d.top = top; d.left = left;
    d.scale = scale;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (rep_dtype == EVREP_F64) return detin_launch<double>(d, rep, B, stream);
    return detin_launch<float>(d, rep, B, stream);
}

}  // extern "C"
