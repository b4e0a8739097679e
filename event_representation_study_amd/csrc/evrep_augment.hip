// evrep_augment.hip -- N-ImageNet's event front end and base_augment("train") on the device
// (n_imagenet/real_cnn_model/data/imagenet.py: load_event :30-57, reshape_event_no_sample :104-108, slice_event :60-84,
// random_time_flip / random_flip_events_along_x / random_shift_events :1140-1173), for all windows of a batch in three launches:
//
//   k_nimg_pass<false>  count: one lane per row of the concatenated windows, cut into kAugSlices contiguous slices (a slice may
//                       straddle windows).  The keep predicate comes from the row itself; ballot + popcount give the slice's
//                       kept count, and the window table receives min p, the last sliced row, the first and last kept row
//                       (integer atomicMin / atomicMax) and the kept count (integer atomicAdd): no result depends on scheduling.
//   k_nimg_scan         one workgroup: slice counts -> exclusive prefix; window counts -> offsets_out; per window the first
//                       and last output time and the status word.
//   k_nimg_pass<true>   write: the transform again; row r of window b goes to offsets_out[b] + r, of a time-flipped window to
//                       offsets_out[b] + kept_b - 1 - r (a wave's stores are one contiguous block either way).
//
// Every float64 step is the reference's single IEEE operation (the build has -ffp-contract=off -fno-fast-math; the divisions
// are the correctly rounded ones).  Sizes are read on the device; nothing returns to the host between the launches.
#pragma once
#include "evrep_common.h"

namespace evrep {

constexpr int kAugSlices = 1024;
constexpr int kAugThreads = 1024;
constexpr int kAugWaves = kAugThreads / kWave;

// one entry per window; cleared to 0xFF bytes by the caller, so every field starts at the identity of its reduction
struct AugWindow {
    uint32_t pmin;        // atomicMin of p ^ 0x80000000 (order-preserving), over ALL rows of the window
    int32_t last_sliced;  // atomicMax of the window row index, rows inside the slice; -1: none
    uint32_t first_kept;  // atomicMin, kept rows; 0xFFFFFFFF: none
    int32_t last_kept;    // atomicMax, kept rows; -1: none
    double t_first;       // t' of the first / last OUTPUT row (k_nimg_scan)
    double t_last;
    double t_flip;        // T of a time-flipped window: t of its last sliced row (k_nimg_scan)
};
static_assert(sizeof(AugWindow) == 40, "AugWindow layout");

// scratch: uint32 [kAugSlices + 1] slice counts / prefix | AugWindow [B] | uint32 [B] kept counts (cleared to 0)
__host__ __device__ inline size_t aug_off_table() { return ((size_t)(kAugSlices + 1) * sizeof(uint32_t) + 255) & ~(size_t)255; }
__host__ __device__ inline size_t aug_off_kept(int B) { return aug_off_table() + (size_t)B * sizeof(AugWindow); }
__host__ __device__ inline size_t aug_scratch_bytes(int B) { return aug_off_kept(B) + (size_t)B * sizeof(uint32_t); }

struct AugArgs {
    const int4 *ev;
    const int64_t *off;
    const int64_t *t_base;
    const evrep_nimg_params *par;
    double sx, sy, res_w, res_h;
    int B;
    uint32_t mode;
};

__device__ inline bool aug_bad_slice(const evrep_nimg_params &p, int64_t n) { return p.s0 < 0 || p.s0 > p.s1 || p.s1 > n; }

// load_event's time (:51): the absolute integer time as float64, divided by 1e6
__device__ inline double aug_time(const AugArgs &a, int b, int t) { return (double)((a.t_base ? a.t_base[b] : 0) + (int64_t)t) / 1000000.0; }

__device__ inline int aug_p(const AugArgs &a, int p) { return (a.mode & EVREP_NIMG_P_UINT8) ? (p & 0xFF) : p; }

// the row's coordinates behind reshape, x flip and shift; `sliced`: inside the index range and the strict time predicate;
// returns keep = sliced and (eval mode or inside the frame)
__device__ inline bool aug_row(const AugArgs &a, const evrep_nimg_params &p, int64_t r, const int4 &e, double ts, double &x, double &y,
                               bool &sliced) {
    sliced = r >= p.s0 && r < p.s1 && ts > p.t_lo && ts < p.t_hi;
    x = (double)e.x * a.sx;
    y = (double)e.y * a.sy;
    if (p.flags & EVREP_AUG_X_FLIP) x = (a.res_w - 1.0) - x;
    if (!(a.mode & EVREP_NIMG_TRAIN)) return sliced;
    x = x + (double)p.x_shift;
    y = y + (double)p.y_shift;
    return sliced && x >= 0.0 && x < a.res_w && y >= 0.0 && y < a.res_h;
}

__device__ inline void aug_slice(const int64_t *__restrict__ off, int B, int s, int64_t &lo, int64_t &hi) {
    const int64_t first = off[0], n = off[B] - first;
    const int64_t per = (n + kAugSlices - 1) / kAugSlices;
    lo = first + min((int64_t)s * per, n);
    hi = min(lo + per, first + n);
}

// grid (kAugSlices), 1024 threads
template <bool WRITE>
__global__ __launch_bounds__(kAugThreads) void k_nimg_pass(AugArgs a, uint32_t *__restrict__ slice_cnt, AugWindow *__restrict__ table,
                                                          uint32_t *__restrict__ kept_cnt, const int64_t *__restrict__ off_out,
                                                          int4 *__restrict__ ev_out, double *__restrict__ t_out,
                                                          double *__restrict__ tn_out, double2 *__restrict__ xy_out) {
    __shared__ uint32_t wave_tot[kAugWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo, hi;
    aug_slice(a.off, a.B, blockIdx.x, lo, hi);
    uint32_t base = WRITE ? slice_cnt[blockIdx.x] : 0u;
    int b_lo = lo < hi ? find_window(a.off, 0, a.B - 1, lo) : 0;                                  // uniform
    for (int64_t r0 = lo; r0 < hi; r0 += kAugThreads) {                                             // uniform
        const int64_t r_end = min(r0 + kAugThreads, hi) - 1;
        const int b_hi = find_window(a.off, b_lo, a.B - 1, r_end);                              // uniform
        const int64_t i = r0 + tid;
        const bool live = i < hi;
        bool keep = false, sliced = false, bad = true;
        int b = b_lo, pv = 0;
        int64_t r = 0;
        double x = 0.0, y = 0.0, ts = 0.0;
        evrep_nimg_params p = {};
        if (live) {
            b = find_window(a.off, b_lo, b_hi, i);
            const int64_t beg = a.off[b];
            r = i - beg;
            p = a.par[b];
            bad = aug_bad_slice(p, a.off[b + 1] - beg);
            if (!bad) {                                    // (nothing of a window with a bad slice is read)
                const int4 e = a.ev[i];
                pv = aug_p(a, e.w);
                ts = aug_time(a, b, e.z);
                keep = aug_row(a, p, r, e, ts, x, y, sliced);
            }
        }
        const uint64_t kmask = __ballot(keep);
        const uint32_t wave_pre = (uint32_t)__popcll(kmask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wave] = (uint32_t)__popcll(kmask);
        if (!WRITE) {
            // the window table: one set of atomics per wave where the wave lies inside one window, else per lane
            const int b0 = __shfl(b, 0, 64);
            const bool one = __ballot(live && !bad && b != b0) == 0ull;
            const uint64_t vmask = __ballot(live && !bad), smask = __ballot(sliced);
            if (one) {
                uint32_t pm = (live && !bad) ? ((uint32_t)pv ^ 0x80000000u) : 0xFFFFFFFFu;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) pm = min(pm, (uint32_t)__shfl_xor((int)pm, o, 64));
                const int rw = __shfl((int)r, 0, 64);   // lane 0's window row; lane l holds rw + l
                if (lane == 0 && vmask) {
                    // (lane 0 is live and in window b0 whenever any lane of the wave is)
                    AugWindow *w = table + b0;
                    atomicMin(&w->pmin, pm);
                    if (smask) atomicMax(&w->last_sliced, (int32_t)(rw + 63 - __builtin_clzll(smask)));
                    if (kmask) {
                        atomicMin(&w->first_kept, (uint32_t)(rw + __builtin_ctzll(kmask)));
                        atomicMax(&w->last_kept, (int32_t)(rw + 63 - __builtin_clzll(kmask)));
                        atomicAdd(kept_cnt + b0, (uint32_t)__popcll(kmask));
                    }
                }
            } else if (live && !bad) {
                AugWindow *w = table + b;
                atomicMin(&w->pmin, (uint32_t)pv ^ 0x80000000u);
                if (sliced) atomicMax(&w->last_sliced, (int32_t)r);
                if (keep) {
                    atomicMin(&w->first_kept, (uint32_t)r);
                    atomicMax(&w->last_kept, (int32_t)r);
                    atomicAdd(kept_cnt + b, 1u);
                }
            }
        }
        __syncthreads();
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kAugWaves; ++w) {
            const uint32_t t = wave_tot[w];
            if (w < wave) pre += t;
            tot += t;
        }
        __syncthreads();
        if (WRITE && keep) {
            const AugWindow w = table[b];
            const bool flip = (p.flags & EVREP_AUG_TIME_FLIP) != 0;
            const int64_t g = (int64_t)base + pre + wave_pre;                                  // stable position among all kept rows
            const int64_t ob = off_out[b], dst = flip ? ob + off_out[b + 1] - 1 - g : g;
            // load_event's zero-polarity rule (:54-55) over the WHOLE window, then the flip's inversion (:1170)
            if ((int32_t)(w.pmin ^ 0x80000000u) >= 0 && pv <= 0) pv = -1;
            if (flip) { pv = -pv; ts = w.t_flip - ts; }
            ev_out[dst] = make_int4((int)x, (int)y, 0, (pv > 0) - (pv < 0));
            t_out[dst] = ts;
            tn_out[dst] = (ts - w.t_first) / (w.t_last - w.t_first);
            if (xy_out) xy_out[dst] = make_double2(x, y);
        }
        base += tot;
        b_lo = b_hi;
    }
    if (!WRITE && tid == 0) slice_cnt[blockIdx.x] = base;
}

// grid (1), 1024 threads
__global__ __launch_bounds__(kAugThreads) void k_nimg_scan(AugArgs a, uint32_t *__restrict__ slice_cnt, AugWindow *__restrict__ table,
                                                          const uint32_t *__restrict__ kept_cnt, int64_t *__restrict__ off_out,
                                                          uint32_t *__restrict__ status_out) {
    __shared__ uint32_t tmp[kAugWaves];
    static_assert(kAugSlices == kAugThreads, "one slice count per thread");
    const int tid = threadIdx.x;
    uint32_t tot;
    const uint32_t v = slice_cnt[tid];
    const uint32_t pre = block_exclusive_scan<kAugWaves>(v, tmp, &tot);
    slice_cnt[tid] = pre;
    if (tid == 0) slice_cnt[kAugSlices] = tot;
    int64_t carry = 0;
    for (int b0 = 0; b0 < a.B; b0 += kAugThreads) {                                            // uniform
        const int b = b0 + tid;
        const uint32_t k = b < a.B ? kept_cnt[b] : 0u;
        const uint32_t kp = block_exclusive_scan<kAugWaves>(k, tmp, &tot);
        if (b < a.B) {
            off_out[b] = carry + kp;
            const evrep_nimg_params p = a.par[b];
            const int64_t beg = a.off[b];
            uint32_t st = 0;
            if (aug_bad_slice(p, a.off[b + 1] - beg)) st |= EVREP_AUG_BAD_SLICE;
            if (k == 0) {
                st |= EVREP_AUG_EMPTY;
            } else {
                AugWindow *w = table + b;
                double tf = aug_time(a, b, a.ev[beg + w->first_kept].z), tl = aug_time(a, b, a.ev[beg + w->last_kept].z);
                if (p.flags & EVREP_AUG_TIME_FLIP) {       // the output starts at the last kept row: t' = T - t
                    const double T = aug_time(a, b, a.ev[beg + w->last_sliced].z);
                    const double f = T - tl;
                    tl = T - tf;
                    tf = f;
                    w->t_flip = T;
                }
                w->t_first = tf;
                w->t_last = tl;
                if (tl == tf) st |= EVREP_AUG_FLAT_TIME;
            }
            status_out[b] = st;
        }
        carry += tot;
    }
    if (tid == 0) off_out[a.B] = carry;
}

}  // namespace evrep
