// evrep_est_prep.hip -- the EST quantisation layer's event preparation on the device.
//
// The layer's caller hands float32 rows [x, y, t, p, b] grouped by batch index b (ev-YOLOv6/yolov6/models/learned_repr.py:143-179
// works on them where they are).  The builders want int32 rows {x, y, 0, p}, offsets per batch item and tn = t / t.max() per item
// (:145, :159-160, :164, :170).  Two streaming launches, grid-stride, sized by n and not by B:
//   k_est_prep_scan   boundaries -> offsets, per-item maximum of t, validation -> status
//   k_est_prep_write  tn = t / max (one correctly rounded float32 division), int32 rows in one 16-byte store per event
// offsets: the lane of event i compares b_i with b_(i-1) (b_(-1) = -1) and, where b_i is larger, writes offsets[k] = i for every k in
//   (b_(i-1), b_i]; the last event's lane writes offsets[k] = n for k in (b_(n-1), B].  For grouped b every entry is written exactly
//   once: no initialisation, no sort, no scan, and skipped indices come out as empty items.  The indices used are clamped to
//   [-1, B-1], so a stream that is refused through the status word still writes inside offsets[0..B] only (an entry may then be
//   written more than once, and the number of stores is the sum of the upward jumps of b: B for every valid stream).
// maximum: each t becomes the usual monotone uint32 image of a float32 (negatives: all bits flipped, the rest: sign bit set; the top
//   key 0xFFFFFFFF is kept for NaN, which poisons its item as torch.max does).  A wave reduces first -- a plain butterfly when a
//   ballot shows that its lanes share one item, per item otherwise -- and issues one integer atomicMax per (wave, item).  Integer
//   maxima do not depend on the order, so two calls give the same bits; no floating-point atomic is used.
// The 20-byte rows are read with five dword loads per lane: a wave's 64 rows are 1 280 contiguous bytes, so the five loads touch
// the same ten or eleven 128-byte lines back to back and every byte comes from HBM once per launch.
// scratch: uint32 [B] keys, uint32 [1] status accumulator; cleared by the call itself (one hipMemsetAsync on the stream).
#include "evrep_capi_shared.h"

namespace evrep {

constexpr int kEpThreads = 256;
constexpr int kEpMaxGroups = 2048;      // 256 CUs x 8 workgroups; longer streams stride
constexpr int kEpMaxB = 65535;          // what evrep_plan_init accepts
constexpr uint32_t kEpNanKey = 0xFFFFFFFFu;

static_assert(kEpThreads % kWave == 0, "a workgroup is a whole number of waves");

__device__ inline uint32_t ep_key(float t) {
    if (t != t) return kEpNanKey;
    const uint32_t u = __float_as_uint(t);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ inline float ep_unkey(uint32_t k) {
    if (k == kEpNanKey) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// the batch item of b, clamped to [-1, B-1] (NaN: -1); *bad: b is not one of 0 .. B-1
__device__ inline int ep_item(float b, int B, bool *bad) {
    *bad = !(b >= 0.0f && b < (float)B && b == truncf(b));
    return (int)floorf(fminf(fmaxf(b, -1.0f), (float)(B - 1)));
}

// (int)v as .long() truncates, defined for every v (NaN and values beyond int32 saturate; such events are refused anyway)
__device__ inline int ep_trunc(float v) { return (int)fminf(fmaxf(v, -2147483648.0f), 2147483520.0f); }

__device__ inline uint32_t ep_wave_max(uint32_t v) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m, kWave);
        v = o > v ? o : v;
    }
    return v;
}

__device__ inline uint32_t ep_wave_or(uint32_t v) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v |= (uint32_t)__shfl_xor((int)v, m, kWave);
    return v;
}

__global__ __launch_bounds__(kEpThreads) void k_est_prep_scan(const float *__restrict__ ev, int64_t n, int B, int H, int W,
                                                              int64_t *__restrict__ offsets, uint32_t *__restrict__ keys) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t stride = (int64_t)gridDim.x * kEpThreads;
    uint32_t st = 0;
    // base is the same in all lanes of a wave: every shuffle and ballot below is executed by the whole wave
    for (int64_t base = (int64_t)blockIdx.x * kEpThreads + (threadIdx.x - lane); base < n; base += stride) {
        const int64_t i = base + lane;
        const bool live = i < n;
        float x = 0.0f, y = 0.0f, t = 0.0f, p = 0.0f, b = 0.0f;
        if (live) {
            const float *r = ev + i * 5;
            x = r[0]; y = r[1]; t = r[2]; p = r[3]; b = r[4];
        }
        float bprev = __shfl_up(b, 1, kWave);
        if (lane == 0 && base > 0) bprev = ev[(base - 1) * 5 + 4];
        bool bad, badprev;
        const int g = ep_item(b, B, &bad);
        const int gprev = i > 0 ? ep_item(bprev, B, &badprev) : -1;
        if (live) {
            if (i > 0 && b < bprev) st |= EVREP_EST_PREP_DESCENDING;
            if (bad) st |= EVREP_EST_PREP_BAD_INDEX;
            if (!(p == 0.0f || p == 1.0f)) st |= EVREP_EST_PREP_BAD_POLARITY;
            if (!(x > -1.0f && x < (float)W && y > -1.0f && y < (float)H)) st |= EVREP_EST_PREP_OUT_OF_FRAME;   // trunc(x) in [0, W)
            for (int k = gprev + 1; k <= g; ++k) offsets[k] = i;               // 0 <= k <= B - 1
            if (i == n - 1)
                for (int k = g + 1; k <= B; ++k) offsets[k] = n;
        }
        const uint32_t key = live ? ep_key(t) : 0u;
        const int gi = g < 0 ? 0 : g;                                          // the keys' index: 0 .. B - 1
        const unsigned long long act = __ballot(live);                         // lane 0 is live: base < n
        const int g0 = __shfl(gi, 0, kWave);
        if (__ballot(live && gi == g0) == act) {                               // one item in the wave
            const uint32_t m = ep_wave_max(key);
            if (lane == 0) atomicMax(keys + g0, m);
        } else {
            unsigned long long todo = act;
            while (todo) {
                const int src = __ffsll((long long)todo) - 1;
                const int gk = __shfl(gi, src, kWave);
                const bool mine = live && gi == gk;
                const uint32_t m = ep_wave_max(mine ? key : 0u);
                if (lane == src) atomicMax(keys + gk, m);
                todo &= ~__ballot(mine);
            }
        }
    }
    st = ep_wave_or(st);
    if (lane == 0 && st) atomicOr(keys + B, st);
}

__global__ __launch_bounds__(kEpThreads) void k_est_prep_write(const float *__restrict__ ev, int64_t n, int B,
                                                               const uint32_t *__restrict__ keys, int4 *__restrict__ rows,
                                                               float *__restrict__ tnorm, uint32_t *__restrict__ status) {
    if (blockIdx.x == 0 && threadIdx.x == 0) status[0] = keys[B];
    const int64_t stride = (int64_t)gridDim.x * kEpThreads;
    for (int64_t i = (int64_t)blockIdx.x * kEpThreads + threadIdx.x; i < n; i += stride) {
        const float *r = ev + i * 5;
        const float x = r[0], y = r[1], t = r[2], p = r[3], b = r[4];
        bool bad;
        const int g = ep_item(b, B, &bad);
        const float tmax = ep_unkey(keys[g < 0 ? 0 : g]);
        tnorm[i] = __fdiv_rn(t, tmax);                                         // t / t.max()  (:159-160); 0 / 0 = NaN as there
        rows[i] = make_int4(ep_trunc(x), ep_trunc(y), 0, ep_trunc(p));         // idx.long() truncates  (:170)
    }
}

}  // namespace evrep

using namespace evrep;
using evrep_host::hip_check;

// scratch: uint32 [B] keys, uint32 [1] status accumulator
static inline size_t est_prep_scratch_bytes(int32_t B) { return ((size_t)B + 1) * sizeof(uint32_t); }

extern "C" {

size_t evrep_est_prepare_scratch_bytes(int64_t n, int32_t B) {
    if (n <= 0 || B <= 0 || B > kEpMaxB) return 0;
    return up256(est_prep_scratch_bytes(B));
}

int evrep_est_prepare(const float *events5, int64_t n, int32_t B, int32_t H, int32_t W, int32_t *rows, int64_t *offsets,
                      float *tnorm, uint32_t *status, void *scratch, void *stream_) {
    if (n <= 0 || B <= 0 || B > kEpMaxB || H < 1 || W < 1 || H > EVREP_MAX_DIM || W > EVREP_MAX_DIM) return EVREP_EINVAL;
    if (bad_ptr(events5, 4) || bad_ptr(rows, 16) || bad_ptr(offsets, 8) || bad_ptr(tnorm, 4) || bad_ptr(status, 4) || bad_ptr(scratch, 4))
        return EVREP_EINVAL;
    hipStream_t stream = as_stream(stream_);
    uint32_t *keys = static_cast<uint32_t *>(scratch);
    if (int rc = hip_check(hipMemsetAsync(keys, 0, est_prep_scratch_bytes(B), stream), "hipMemsetAsync(est_prepare)")) return rc;
    const int64_t want = (n + kEpThreads - 1) / kEpThreads;
    const int groups = (int)(want < kEpMaxGroups ? want : kEpMaxGroups);
    k_est_prep_scan<<<groups, kEpThreads, 0, stream>>>(events5, n, B, H, W, offsets, keys);
    LAUNCH_CHECK("k_est_prep_scan");
    k_est_prep_write<<<groups, kEpThreads, 0, stream>>>(events5, n, B, keys, reinterpret_cast<int4 *>(rows), tnorm, status);
    LAUNCH_CHECK("k_est_prep_write");
    return EVREP_OK;
}

}  // extern "C"
