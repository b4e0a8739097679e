// evrep_windows.hip -- windows cut from a DEVICE-RESIDENT recording: the time-to-index search of the ev-licious handle
// (ev-licious/src/evlicious/io/h5_event_handle.py:10-11) and the gather of B source ranges of the recording's
// structure-of-arrays columns (x u16, y u16, t i64, p i8: io/utils/events.py:7-8) into the packed int32 [x, y, t - base, p]
// rows an EventBatch consumes.
//
// k_time_to_index: ONE WAVEFRONT PER QUERY, a 64-ary search.  A lane-private binary search through HBM is a chain of
// log2(n) dependent loads (VERDICT.md item 7 measures that shape in k_ts_cuts: 16 probes, 12-14 us); here every round is one
// load per lane, all 64 in flight together, a ballot picks the sub-range, and the last round reads 64 consecutive entries:
// ceil(log64 n) dependent loads, 4 for 10^7 events.
//
// k_windows_gather: the work is cut over OUTPUT ROWS, not over windows: a wave owns kGatherWaveRows consecutive destination
// rows and finds the windows they belong to in the offsets table (the same 64-ary search), so one window of 10^6 events and
// a thousand windows of 50 events fill the chip alike.  A fixed grid strides over the rows: the total lives in
// dst_offsets[B] on the device and is never needed on the host.
#pragma once
#include "evrep_common.h"
#include "evrep_wave_search.h"

namespace evrep {

constexpr int kGatherRowsPerLane = 4;
constexpr int kGatherWaveRows = kWave * kGatherRowsPerLane;                 // 256 consecutive rows per wave
constexpr int kGatherSpan = kGatherWaveRows * (kWinThreads / kWave);       // 1024 rows per workgroup and stride step
constexpr int kGatherGrid = 2048;                                           // 256 CUs x 8 workgroups

// grid ceil(nq / 4), 256 threads: wave w of the grid answers query w.
__global__ __launch_bounds__(kWinThreads) void k_time_to_index(const int64_t *__restrict__ t, int64_t n,
                                                               const int64_t *__restrict__ queries, int64_t nq,
                                                               int64_t *__restrict__ out_idx) {
    const int64_t w = ((int64_t)blockIdx.x * kWinThreads + threadIdx.x) / kWave;
    if (w >= nq) return;                                             // (wave-uniform: a wave is 64 consecutive threads)
    const int64_t q = wave_uniform(queries[w]);
    const int64_t i = wave_upper_bound(t, n, q);
    if ((threadIdx.x & (kWave - 1)) == 0) out_idx[w] = i;
}

// A range the recording does not hold: nothing of it is read.
__device__ inline bool range_ok(int64_t a, int64_t b, int64_t n) { return a >= 0 && a <= b && b <= n; }

__device__ inline int64_t window_base(const int64_t *__restrict__ t, int64_t a, int64_t b, int64_t n, int mode,
                                      const int64_t *__restrict__ base_in, int64_t win) {
    if (mode == EVREP_REBASE_FIRST) return (range_ok(a, b, n) && a < b) ? t[a] : 0;
    if (mode == EVREP_REBASE_GIVEN) return base_in[win];
    return 0;
}

// grid kGatherGrid, 256 threads.  status must be cleared by the caller (the C entry point does).
// Part 1, one thread per window over the whole grid: base_out[b], and EVREP_WST_BAD_RANGE for a range outside the recording.
// Part 2, the rows: the workgroup strides over spans of kGatherSpan destination rows; each wave takes kGatherWaveRows of
// them, looks up the windows of its first and its last row with the wave search, and each lane then finds its row's window
// between the two (no probe at all where the wave lies inside one window, the common case).  Row r of window b is source
// event i0[b] + (r - off[b]): consecutive lanes read consecutive entries of x, y, t and p, and store consecutive 16-byte
// rows.  A source index outside [i0[b], i1[b]) -- offsets that do not match the ranges -- is never read
// (EVREP_WST_BAD_OFFSETS).
__global__ __launch_bounds__(kWinThreads) void k_windows_gather(const uint16_t *__restrict__ x, const uint16_t *__restrict__ y,
                                                                const int64_t *__restrict__ t, const int8_t *__restrict__ p,
                                                                int64_t n, const int64_t *__restrict__ i0,
                                                                const int64_t *__restrict__ i1, const int64_t *__restrict__ off,
                                                                int B, int mode, const int64_t *__restrict__ base_in,
                                                                int4 *__restrict__ out, int64_t *__restrict__ base_out,
                                                                uint32_t *__restrict__ status) {
    for (int64_t b = (int64_t)blockIdx.x * kWinThreads + threadIdx.x; b < B; b += (int64_t)gridDim.x * kWinThreads) {
        const int64_t a = i0[b], e = i1[b];
        base_out[b] = window_base(t, a, e, n, mode, base_in, b);
        if (!range_ok(a, e, n)) atomicOr(&status[b], EVREP_WST_BAD_RANGE);
    }
    const int64_t row0 = off[0], total = off[B];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int64_t span = row0 + (int64_t)blockIdx.x * kGatherSpan; span < total; span += (int64_t)gridDim.x * kGatherSpan) {
        const int64_t wfirst = span + (int64_t)wave * kGatherWaveRows;
        if (wfirst >= total) continue;                               // (wave-uniform)
        const int64_t wlast = (wfirst + kGatherWaveRows < total ? wfirst + kGatherWaveRows : total) - 1;
        // the window of row r: the last b with off[b] <= r, i.e. (first index with off > r) - 1, held inside [0, B - 1]
        int64_t blo = wave_upper_bound(off, (int64_t)B + 1, wfirst) - 1;
        int64_t bhi = wave_upper_bound(off, (int64_t)B + 1, wlast) - 1;
        blo = blo < 0 ? 0 : (blo > B - 1 ? B - 1 : blo);
        bhi = bhi < blo ? blo : (bhi > B - 1 ? B - 1 : bhi);
#pragma unroll
        for (int k = 0; k < kGatherRowsPerLane; ++k) {
            const int64_t r = wfirst + k * kWave + lane;
            if (r > wlast) break;
            int64_t lo = blo, hi = bhi;                              // the last b in [lo, hi] with off[b] <= r
            while (lo < hi) {
                const int64_t mid = (lo + hi + 1) >> 1;
                if (off[mid] <= r) lo = mid; else hi = mid - 1;
            }
            const int64_t b = lo;
            const int64_t a = i0[b], e = i1[b];
            if (!range_ok(a, e, n)) continue;                        // flagged in part 1: nothing is copied
            const int64_t src = a + (r - off[b]);
            if (src < a || src >= e) {
                atomicOr(&status[b], EVREP_WST_BAD_OFFSETS);
                continue;
            }
            const int64_t base = window_base(t, a, e, n, mode, base_in, b);
            const int64_t tv = t[src];
            int64_t d;
            int32_t tz;
            if (__builtin_sub_overflow(tv, base, &d)) d = tv >= 0 ? INT64_MAX : INT64_MIN;
            if (d > INT32_MAX || d < INT32_MIN) {
                // the row is still written, saturated; the host raises (gen1_h5.py's int64_to_int32: loud, never wrapped)
                atomicOr(&status[b], EVREP_WST_T_OVERFLOW);
                tz = d > 0 ? INT32_MAX : INT32_MIN;
            } else {
                tz = (int32_t)d;
            }
            out[r] = make_int4((int)x[src], (int)y[src], tz, (int)p[src]);   // p as stored: Events.__init__ has mapped 0 to -1
        }
    }
}

}  // namespace evrep
