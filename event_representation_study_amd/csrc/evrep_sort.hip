// evrep_sort.hip -- N-ImageNet's sorted timestamp image (n_imagenet/real_cnn_model/data/imagenet.py:513-838, reshape_then_acc_sort)
// for the B windows of a batch: the per-event time index in front of k_polstats, and the image statements behind it.
//
// TIME INDEX (:521-538), three launches in the count / scan / write structure of evrep_augment.hip:
//   k_ti_pass<false>  count: one lane per event of the concatenated windows, cut into kTiSlices contiguous slices (a slice may
//                     straddle windows).  idx = (int64)(t * 1e6), one IEEE multiply and a truncation.  An event is a HEAD when it
//                     opens its window or its idx differs from the event in front of it (torch.unique_consecutive); ballot +
//                     popcount give the slice's head count, a window's first event records the slice it lies in and the
//                     inclusive head count there, and an idx below its predecessor's sets the window's status bit.
//   k_ti_scan         one workgroup: slice counts -> exclusive prefix; the windows' first events -> global head counts; windows
//                     without events get their status bit.
//   k_ti_pass<true>   write: float64 of idx itself, or of the consecutive rank = heads up to the event - heads up to its window's
//                     first event, so the scan restarts at every window whatever the neighbouring windows hold.
//
// IMAGE, k_sort_image, one workgroup per (window, polarity class) on the [FLAG, TMAX] pairs k_polstats wrote.  strict = 0: TMAX as
// it is (the reference's min-max of the hot pixels is discarded, and its float64 quantisation of an integer returns the integer).
// strict = 1: the dense rank of the hot pixels' TMAX through the pair sort of evrep_ranksort.h -- every pixel without an event
// takes a key below all others, and rank and count are corrected by one where such a pixel exists -- then rank / (U - 1) as one
// correctly rounded division and the quantisations round_half_even(v * q) / q as separate float32 operations (the library is
// built with -ffp-contract=off).  Nothing here waits for the device or reads a size on the host.
#pragma once
#include "evrep_common.h"
#include "evrep_ranksort.h"

namespace evrep {

constexpr int kTiSlices = 256;
constexpr int kTiThreads = 1024;                      // the tile of one round of a slice
constexpr int kTiWaves = kTiThreads / kWave;

// scratch: uint32 [kTiSlices + 1] slice head counts / prefix | uint32 [B] head count at the window's first event | uint32 [B] its slice
__host__ __device__ inline size_t ti_off_start() { return ((size_t)(kTiSlices + 1) * sizeof(uint32_t) + 255) & ~(size_t)255; }
__host__ __device__ inline size_t ti_off_slice(int B) { return ti_off_start() + (((size_t)B * sizeof(uint32_t) + 255) & ~(size_t)255); }
__host__ __device__ inline size_t ti_scratch_bytes(int B) { return ti_off_slice(B) + (((size_t)B * sizeof(uint32_t) + 255) & ~(size_t)255); }

struct TiArgs {
    const double *t;
    const int64_t *off;
    int B;
    int mode;             // EVREP_TIME_INDEX_RAW / EVREP_TIME_INDEX_RANK
};

// (event_tensor[:, 2] * TIME_SCALE).long()
__device__ inline int64_t ti_index(double t) { return (int64_t)(t * 1000000.0); }

__device__ inline void ti_slice(const int64_t *__restrict__ off, int B, int s, int64_t &lo, int64_t &hi) {
    const int64_t first = off[0], n = off[B] - first;
    const int64_t per = (n + kTiSlices - 1) / kTiSlices;
    lo = first + min((int64_t)s * per, n);
    hi = min(lo + per, first + n);
}

// grid (kTiSlices), 1024 threads
template <bool WRITE>
__global__ __launch_bounds__(kTiThreads) void k_ti_pass(TiArgs a, uint32_t *__restrict__ slice_cnt, uint32_t *__restrict__ win_start,
                                                       uint32_t *__restrict__ win_slice, double *__restrict__ out,
                                                       uint32_t *__restrict__ status) {
    __shared__ uint32_t wave_tot[kTiWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t lo, hi;
    ti_slice(a.off, a.B, blockIdx.x, lo, hi);
    uint32_t base = WRITE ? slice_cnt[blockIdx.x] : 0u;          // heads in front of this round: of all slices / of this one
    int b_lo = lo < hi ? find_window(a.off, 0, a.B - 1, lo) : 0;                                    // uniform
    for (int64_t r0 = lo; r0 < hi; r0 += kTiThreads) {                                              // uniform
        const int64_t r_end = min(r0 + kTiThreads, hi) - 1;
        const int b_hi = find_window(a.off, b_lo, a.B - 1, r_end);                                  // uniform
        const int64_t i = r0 + tid;
        const bool live = i < hi;
        bool head = false, first = false, dec = false;
        int b = b_lo;
        int64_t idx = 0;
        if (live) {
            b = find_window(a.off, b_lo, b_hi, i);
            first = i == a.off[b];
            idx = ti_index(a.t[i]);
            head = true;
            if (!first) {
                const int64_t prev = ti_index(a.t[i - 1]);
                head = idx != prev;
                dec = idx < prev;
            }
        }
        const uint64_t hmask = __ballot(head);
        const uint32_t wave_pre = (uint32_t)__popcll(hmask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wave] = (uint32_t)__popcll(hmask);
        if (!WRITE && dec) atomicOr(status + b, EVREP_SORT_DECREASING);
        __syncthreads();
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kTiWaves; ++w) {
            const uint32_t t = wave_tot[w];
            if (w < wave) pre += t;
            tot += t;
        }
        __syncthreads();
        const uint32_t incl = base + pre + wave_pre + (head ? 1u : 0u);
        if (!WRITE) {
            if (first) {
                win_start[b] = incl;
                win_slice[b] = blockIdx.x;
            }
        } else if (live) {
            gstore_f64(out + i, a.mode == EVREP_TIME_INDEX_RANK ? (double)(incl - win_start[b]) : (double)idx);
        }
        base += tot;
        b_lo = b_hi;
    }
    if (!WRITE && tid == 0) slice_cnt[blockIdx.x] = base;
}

// grid (1), 1024 threads
__global__ __launch_bounds__(kTiThreads) void k_ti_scan(TiArgs a, uint32_t *__restrict__ slice_cnt, uint32_t *__restrict__ win_start,
                                                       const uint32_t *__restrict__ win_slice, uint32_t *__restrict__ status) {
    __shared__ uint32_t tmp[kTiWaves];
    static_assert(kTiSlices <= kTiThreads, "one slice count per thread");
    const int tid = threadIdx.x;
    uint32_t tot;
    const uint32_t v = tid < kTiSlices ? slice_cnt[tid] : 0u;
    const uint32_t pre = block_exclusive_scan<kTiWaves>(v, tmp, &tot);
    if (tid < kTiSlices) slice_cnt[tid] = pre;
    if (tid == 0) slice_cnt[kTiSlices] = tot;
    __syncthreads();                                                // the prefixes are read across threads below
    for (int b = tid; b < a.B; b += kTiThreads) {
        if (a.off[b + 1] - a.off[b] <= 0) status[b] |= EVREP_SORT_EMPTY;          // (the count launch is over: nobody else writes it)
        else win_start[b] += slice_cnt[win_slice[b]];
    }
}

// ------------------------------------------------------------------------------------------------------------- the image
struct SortImageArgs {
    const float *prim;          // (B, npx, 2K): [FLAG, TMAX] per class
    float *out;                 // (B, K * (use_image + max(nq, 1)), npx)
    uint32_t *status;           // (B), OR-ed into
    char *scratch;              // four uint32 arrays of rank_array_bytes(B * K * npx) each (strict only)
    int32_t B, K, npx;
    int32_t strict, use_image, nq;
    float q[EVREP_SORT_MAX_Q];
};

// grid (B * K), 1024 threads
__global__ __launch_bounds__(kDistThreads) void k_sort_image(const SortImageArgs a) {
    __shared__ RankSortLds lds;
    const int tid = threadIdx.x;
    const int seg = blockIdx.x, b = seg / a.K, k = seg - b * a.K;
    const size_t C2 = 2u * (size_t)a.K, npx = (size_t)a.npx;
    const float *pix = a.prim + (size_t)b * npx * C2 + 2u * (size_t)k;        // pixel i: pix[i * C2] = FLAG, pix[i * C2 + 1] = TMAX
    const int nsort = a.nq > 0 ? a.nq : 1;
    float *img = a.out + (size_t)seg * (size_t)(a.use_image + nsort) * npx;   // this class's channels: [image?] + sort channels
    float *srt = img + (a.use_image ? npx : 0);

    if (!a.strict) {
        uint32_t positive = 0;
        for (size_t i = tid; i < npx; i += kDistThreads) {
            const float f = pix[i * C2], v = pix[i * C2 + 1];
            if (a.use_image) gstore_f32(img + i, f);
            for (int c = 0; c < nsort; ++c) gstore_f32(srt + (size_t)c * npx + i, v);
            positive |= v > 0.0f ? 1u : 0u;
        }
        uint32_t tot;
        block_exclusive_scan<kDistWaves>(positive, lds.scan_tmp, &tot);
        if (tot == 0 && tid == 0) atomicOr(a.status + b, EVREP_SORT_NO_INDEX << k);   // hot_event_sort.max() of nothing (:597-599)
        return;
    }

    const int64_t n = (int64_t)npx, o0 = (int64_t)seg * n;
    const size_t ab = rank_array_bytes((int64_t)a.B * a.K * n);
    uint32_t *const ka = reinterpret_cast<uint32_t *>(a.scratch) + o0, *const ia = reinterpret_cast<uint32_t *>(a.scratch + ab) + o0;
    uint32_t *const kb = reinterpret_cast<uint32_t *>(a.scratch + 2 * ab) + o0, *const ib = reinterpret_cast<uint32_t *>(a.scratch + 3 * ab) + o0;
    const uint32_t cold_key = rank_key(-1.0f);            // below every hot key: TMAX of a hot pixel is a rank >= 0
    rank_pair_sort([pix, C2, cold_key](int64_t i) { const float *p = pix + (size_t)i * C2; return p[0] > 0.0f ? rank_key(p[1]) : cold_key; },
                   n, ka, ia, kb, ib, lds);

    const uint32_t *ks = kb, *is = ib;
    uint32_t heads = 0;
    for (int64_t i = tid; i < n; i += kDistThreads) heads += (i == 0 || ks[i] != ks[i - 1]) ? 1u : 0u;
    uint32_t ndist;
    block_exclusive_scan<kDistWaves>(heads, lds.scan_tmp, &ndist);
    const uint32_t cold = ks[0] == cold_key ? 1u : 0u;   // a pixel without an event exists: it holds rank 0
    const uint32_t U = ndist - cold;                      // distinct latest indices among the hot pixels
    const float den = (float)(U > 1 ? U - 1u : 1u);
    uint32_t running = 0;                                 // heads in front of this round
    for (int64_t i0 = 0; i0 < n; i0 += kDistThreads) {
        const int64_t i = i0 + tid;
        const uint32_t h = (i < n && (i == 0 || ks[i] != ks[i - 1])) ? 1u : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<kDistWaves>(h, lds.scan_tmp, &tot);
        if (i < n) {
            const bool hot = ks[i] != cold_key;
            // (fs - fs.min()) / (fs.max() - fs.min()) with fs = rank + 1: rank / (U - 1); all zero when U == 1 (:581-586)
            const float s = (hot && U > 1) ? __fdiv_rn((float)(running + ex + h - 1u - cold), den) : 0.0f;
            float *dst = srt + is[i];
            if (a.nq == 0) {
                gstore_f32(dst, s);
            } else {
                for (int c = 0; c < a.nq; ++c) {
                    const float m = s * a.q[c];           // torch.round(sort * q) / q: a multiply, a rounding, a division
                    gstore_f32(dst + (size_t)c * npx, __fdiv_rn(rintf(m), a.q[c]));
                }
            }
        }
        running += tot;
    }
    if (a.use_image) {
        // a polarity without events is the reference's ONE event at pixel (0, 0) (:650-655)
        for (size_t i = tid; i < npx; i += kDistThreads) gstore_f32(img + i, (U == 0 && i == 0) ? 1.0f : pix[i * C2]);
    }
}

}  // namespace evrep
