// evrep_study.hip -- the rows the study's three representations are built from (ERGO-12, EventStack, TORE), formed on the device
// from what evrep_nimg_prepare leaves: the step n_imagenet's reshape_then_optimized / _event_stack / _tore wrappers
// (imagenet.py:1025-1107) take on the host in front of the builders, for the B windows of a batch.
//
//   k_study_reduce  per window: min of (int64)trunc(t) and its max, min x, min y over the float64 xy, and the flags.  All of
//                   them exact and order-free (integer minima of order-preserving keys, an AND of inverted flag bits), so the
//                   partial results of the workgroups a long window is spread over fold through atomics on the window's
//                   64-byte record, whatever the order of arrival.  The records start as all ones (one memset in front).
//   k_study_write   per row: one 16-byte store per wanted row set; per window: the status word and the sample time.
//
// Both kernels walk the concatenated rows [offsets[0], offsets[B]) in slices of 1 024 rows per workgroup, 256 per wave, whatever
// the windows' lengths: a long window is spread over as many workgroups as it has slices, short ones share a wave.  Neither the
// row count nor a window length is known on the host: the grids are fixed and stride.
#pragma once
#include "evrep_common.h"
#include "evrep_wave_search.h"

namespace evrep {

constexpr int kStudyThreads = 256;
constexpr int kStudyBlocks = 2048;     // 256 CUs x 8 workgroups; the rest of the rows by grid stride
constexpr int kStudyRowsPerLane = 4;   // a wave takes 256 consecutive rows, 64 at a time: one window search, and where they lie in
constexpr int kStudyWaveRows = kWave * kStudyRowsPerLane;          // one window (the usual case) one fold into its record
constexpr int kStudyBlockRows = kStudyThreads * kStudyRowsPerLane;

// One window's record in the scratch: four minima as unsigned keys, the flags inverted (all ones = nothing seen yet).
struct StudyWindow {
    unsigned long long tmin_key;    // key of min (int64)trunc(t) over the rows whose t can be cast
    unsigned long long tmax_nkey;   // ~key of the max of the same
    unsigned long long xmin_key;    // key of min x
    unsigned long long ymin_key;    // key of min y
    uint32_t not_flags;             // ~(EVREP_STUDY_* bits seen in some row)
    uint32_t pad[7];
};
static_assert(sizeof(StudyWindow) == 64, "one 64-byte line per window");

__host__ __device__ inline size_t study_scratch_bytes(int32_t B) { return (size_t)B * sizeof(StudyWindow); }

// int64 -> uint64, a < b  <=>  key(a) < key(b)
__device__ inline unsigned long long study_key_i64(int64_t v) { return (unsigned long long)v ^ 0x8000000000000000ull; }
__device__ inline int64_t study_unkey_i64(unsigned long long k) { return (int64_t)(k ^ 0x8000000000000000ull); }
// float64 -> uint64, the usual order-preserving key: negative values have every bit flipped, the others the sign bit set
__device__ inline unsigned long long study_key_f64(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double study_unkey_f64(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// a float64 time the C cast to int64 is defined for: not NaN, below 2^63 in magnitude
__device__ inline bool study_t_ok(double t) { return fabs(t) < 9223372036854775808.0; }
// (int32)trunc(v); INT32_MIN where the C cast is undefined
__device__ inline int32_t study_trunc_i32(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int32_t)v : INT32_MIN; }

__device__ inline unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, kWave);
        v = o < v ? o : v;
    }
    return v;
}
__device__ inline uint32_t wave_or_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v |= __shfl_xor(v, d, kWave);
    return v;
}

// The window of concatenated row i, the last b with off[b] <= i: the 64-ary search of a whole wave (every lane calls it with
// the same row and gets the result).  A lane whose own row lies past that window's end searches on from there (find_window).
__device__ inline int study_window_of(const int64_t *__restrict__ off, int B, int64_t i) {
    const int w = (int)wave_upper_bound(off, (int64_t)B + 1, i) - 1;
    return w < 0 ? 0 : (w > B - 1 ? B - 1 : w);
}

// atomicMin of a key that only ever falls: skipped where the word is seen at or below the key already (the agent-scope
// load may be late, never early: a late value is a larger one)
__device__ inline void study_fold_min(unsigned long long *word, unsigned long long key) {
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(word, key);
}

struct StudyArgs {
    const int4 *rows;           // [x.long(), y.long(), 0, sign p] per row
    const double *t;            // seconds
    const double2 *xy;          // untruncated coordinates (TORE only)
    const int64_t *off;
    int32_t B;
    uint32_t want;
};

// what some rows of ONE window contribute to its record
struct StudyPart {
    unsigned long long kt = ~0ull, nkt = ~0ull, kx = ~0ull, ky = ~0ull;
    uint32_t fl = 0u;
};

// row i of a window that ends at wend and whose last time is t_last, folded into p
__device__ inline void study_row(const StudyArgs &a, bool tore, int64_t i, int64_t wend, double t_last, StudyPart &p) {
    const double t = a.t[i];
    if (study_t_ok(t)) {
        const int64_t ti = (int64_t)t;
        const unsigned long long k = study_key_i64(ti);
        p.kt = k < p.kt ? k : p.kt;
        p.nkt = ~k < p.nkt ? ~k : p.nkt;
        if (!((double)ti <= t_last)) p.fl |= EVREP_STUDY_FUTURE;      // event_stack.py:34-35: int64 t against the float64 last time
    } else {
        p.fl |= EVREP_STUDY_T_RANGE;
    }
    if (i + 1 < wend && !(a.t[i + 1] - t >= 0.0)) p.fl |= EVREP_STUDY_UNORDERED;   // not np.all(np.diff(ts) >= 0)
    if (tore) {
        const double2 c = a.xy[i];
        const unsigned long long kx = study_key_f64(c.x), ky = study_key_f64(c.y);
        p.kx = kx < p.kx ? kx : p.kx;
        p.ky = ky < p.ky ? ky : p.ky;
    }
}

// the lanes' parts (the identity in a lane that holds none of the window) reduced over the wave; lane `leader` folds them into r
__device__ inline void study_fold(StudyWindow *r, bool tore, int lane, int leader, const StudyPart &p) {
    const unsigned long long rt = wave_min_u64(p.kt), rnt = wave_min_u64(p.nkt);
    const uint32_t rf = wave_or_u32(p.fl);
    unsigned long long rx = ~0ull, ry = ~0ull;
    if (tore) { rx = wave_min_u64(p.kx); ry = wave_min_u64(p.ky); }
    if (lane == leader) {
        study_fold_min(&r->tmin_key, rt);
        study_fold_min(&r->tmax_nkey, rnt);
        if (tore) { study_fold_min(&r->xmin_key, rx); study_fold_min(&r->ymin_key, ry); }
        if (rf) atomicAnd(&r->not_flags, ~rf);
    }
}

__global__ __launch_bounds__(kStudyThreads) void k_study_reduce(StudyArgs a, StudyWindow *__restrict__ win) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t beg = a.off[0], end = a.off[a.B];
    const bool tore = (a.want & EVREP_STUDY_TORE) != 0u;
    for (int64_t base = beg + (int64_t)blockIdx.x * kStudyBlockRows; base < end; base += (int64_t)gridDim.x * kStudyBlockRows) {
        const int64_t wave_first = base + (int64_t)(threadIdx.x >> 6) * kStudyWaveRows;
        if (wave_first >= end) continue;                       // wave-uniform
        const int64_t wave_end = wave_first + kStudyWaveRows < end ? wave_first + kStudyWaveRows : end;
        const int w0 = study_window_of(a.off, a.B, wave_first);
        const int64_t wend0 = a.off[w0 + 1];
        if (wave_end <= wend0) {
            // wave-uniform, the usual case: all rows of the wave lie in one window -- one reduction, one fold
            const double t_last = a.t[wend0 - 1];
            StudyPart p;
#pragma unroll
            for (int k = 0; k < kStudyRowsPerLane; ++k) {
                const int64_t i = wave_first + k * kWave + lane;
                if (i < wave_end) study_row(a, tore, i, wend0, t_last, p);
            }
            study_fold(win + w0, tore, lane, 0, p);
            continue;
        }
        // a wave whose rows lie in several windows: per 64 rows one round per window, its lanes reduce among themselves
        for (int k = 0; k < kStudyRowsPerLane; ++k) {
            const int64_t i = wave_first + k * kWave + lane;
            const bool valid = i < wave_end;
            int w = w0;
            StudyPart p;
            if (valid) {
                if (i >= wend0) w = find_window(a.off, w0, a.B - 1, i);
                const int64_t wend = a.off[w + 1];
                study_row(a, tore, i, wend, a.t[wend - 1], p);
            }
            unsigned long long todo = __ballot(valid);
            while (todo) {
                const int first = __ffsll((long long)todo) - 1;
                const int wl = __shfl(w, first, kWave);
                const bool mine = valid && w == wl;
                study_fold(win + wl, tore, lane, first, mine ? p : StudyPart());
                todo &= ~__ballot(mine);
            }
        }
    }
}

// the status word of a window of n rows from its finished record
__device__ inline uint32_t study_status(const StudyWindow &r, int64_t n) {
    if (n <= 0) return EVREP_STUDY_EMPTY;
    uint32_t st = ~r.not_flags & (EVREP_STUDY_FUTURE | EVREP_STUDY_T_RANGE | EVREP_STUDY_UNORDERED);
    if (r.tmin_key != ~0ull) {                                  // some row's time could be cast
        const unsigned long long span = ~r.tmax_nkey - r.tmin_key;      // exact: the keys keep the order and the distance
        if (span > (unsigned long long)INT32_MAX) st |= EVREP_STUDY_T_RANGE;
        if (span == 0ull && !(st & EVREP_STUDY_T_RANGE)) st |= EVREP_STUDY_FLAT;
    }
    return st;
}

__global__ __launch_bounds__(kStudyThreads) void k_study_write(StudyArgs a, const StudyWindow *__restrict__ win, int4 *__restrict__ rows_mdes,
                                                              int4 *__restrict__ rows_stack, int4 *__restrict__ rows_tore,
                                                              double *__restrict__ sample_times, uint32_t *__restrict__ status) {
    // per window: the status word and TORE's sample time, t of the window's last row (imagenet.py:1100)
    for (int64_t b = (int64_t)blockIdx.x * kStudyThreads + threadIdx.x; b < a.B; b += (int64_t)gridDim.x * kStudyThreads) {
        const int64_t n = a.off[b + 1] - a.off[b];
        status[b] = study_status(win[b], n);
        if (sample_times) sample_times[b] = n > 0 ? a.t[a.off[b + 1] - 1] : 0.0;
    }
    const int64_t beg = a.off[0], end = a.off[a.B];
    const int lane = threadIdx.x & (kWave - 1);
    for (int64_t base = beg + (int64_t)blockIdx.x * kStudyBlockRows; base < end; base += (int64_t)gridDim.x * kStudyBlockRows) {
        const int64_t wave_first = base + (int64_t)(threadIdx.x >> 6) * kStudyWaveRows;
        if (wave_first >= end) continue;                       // wave-uniform
        const int64_t wave_end = wave_first + kStudyWaveRows < end ? wave_first + kStudyWaveRows : end;
        const int w0 = study_window_of(a.off, a.B, wave_first);
        const int64_t wend0 = a.off[w0 + 1];
        for (int q = 0; q < kStudyRowsPerLane; ++q) {
            const int64_t i = wave_first + q * kWave + lane;
            if (i >= wave_end) continue;
            const int w = i < wend0 ? w0 : find_window(a.off, w0, a.B - 1, i);
            const StudyWindow r = win[w];
            const int4 e = a.rows[i];
            if (rows_mdes) {
                // [x, y, (int32)((int64)trunc(t) - tmin), p]: mixed_density_event_stack.py:26-33 (the difference wraps as numpy's does)
                const double t = a.t[i];
                int32_t tc = 0;
                if (study_t_ok(t) && r.tmin_key != ~0ull)
                    tc = (int32_t)(uint32_t)((unsigned long long)(int64_t)t - (unsigned long long)study_unkey_i64(r.tmin_key));
                gstore16(rows_mdes + i, make_uint4((uint32_t)e.x, (uint32_t)e.y, (uint32_t)tc, (uint32_t)e.w));
            }
            if (rows_stack) {
                // [x, y, 0, 2 * ((p + 1) // 2) - 1]: imagenet.py:1051 and event_stack.py:18; stacking never reads the time
                gstore16(rows_stack + i, make_uint4((uint32_t)e.x, (uint32_t)e.y, 0u, (uint32_t)(e.w > 0 ? 1 : -1)));
            }
            if (rows_tore) {
                // x - min(x) + 1, y - min(y) + 1 (imagenet.py:1098-1099), each step one float64 rounding, then int() and the
                // builder's 0-based index (tore.py:29-33); the time column is the order marker of events2ToreFeature's float-time
                // branch: the row's index in its window, counted down where the times do not ascend
                const double2 c = a.xy[i];
                const double xs = (c.x - study_unkey_f64(r.xmin_key)) + 1.0, ys = (c.y - study_unkey_f64(r.ymin_key)) + 1.0;
                const int32_t k = (int32_t)(i - a.off[w]);
                const int32_t marker = (~r.not_flags & EVREP_STUDY_UNORDERED) ? -k : k;
                gstore16(rows_tore + i, make_uint4((uint32_t)study_trunc_i32(xs) - 1u, (uint32_t)study_trunc_i32(ys) - 1u, (uint32_t)marker,
                                                   (uint32_t)e.w));
            }
        }
    }
}

}  // namespace evrep
