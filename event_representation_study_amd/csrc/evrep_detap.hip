// evrep_detap.hip -- average precision on the device: yolov6/utils/metrics.py's ap_per_class and compute_ap for the rows the
// evaluator kept resident, from the padded per-batch tensors to p, r, f1 (nc, 1000) and ap (nc, T) with no host loop and no
// host sort.  include/evrep.h states the rules A1-A7 with evrep_det_ap; this file is the launch sequence behind it.
//
//   gather    (evrep_det_ap_gather, per batch)  k_ap_gather_rows: workgroup b sums the clamped counts in front of image b and
//             copies its rows behind the cursor; k_ap_gather_finish (one workgroup, the next launch: every reader of the cursor
//             is done) lists the target classes of the rows whose image lies in [0, B) and moves the cursor.
//   keys      k_ap_keys: row i -> (class << 32 | ~rank_key(conf)), the class nc for a row that takes part in nothing; the rows
//             of a class are counted in LDS and added with integer atomics.  k_ap_targets counts the labels the same way.
//   segments  k_ap_segments (one workgroup): the exclusive scan of the class counts -> where each class's rows start.
//   sort      a stable LSD radix sort of the 64-bit keys, eight bits a pass, the low 32 bits and then the class bits, carrying
//             the row index: per pass k_ap_radix_count (a digit histogram per tile of 2 048 rows), k_ap_radix_scan (ONE
//             workgroup: the exclusive scan over (digit, tile)), k_ap_radix_scatter (a tile's rows in order, 256 a round, wave
//             after wave: wave_match ranks a wave's rows, the digit's running base lives in LDS).  Equal keys keep array order.
//   counts    tpc of A3 as an integer scan over ALL sorted rows, the T thresholds of a row together, with the count in front
//             of the class's first row subtracted where it is read (exact: integers): k_ap_cum_sums (a wave per tile of 512
//             rows, a ballot and a popcount per threshold), k_ap_cum_scan (one workgroup), k_ap_cum_write.
//   mpre      A6's running maximum from the right, segmented by class: k_ap_max_heads (per tile the maximum over the rows of
//             its first row's class), k_ap_max_carry (one workgroup walks the tiles from the last), k_ap_max_write.
//   curves    k_ap_curves: a lane per (class, point of px), A5 as a binary search, p, r and f1 written.  k_ap_area: a wave per
//             (class, threshold) holds the 101 y in LDS and lane 0 adds the 100 terms in ascending order.
//
// Every dependency between workgroups is a launch boundary; no workgroup waits for another inside a launch.  n and m may be
// resident on the device (counts_dev): the grids are sized by the capacities and every kernel reads the true numbers.  Float64
// statements are single operations (-ffp-contract=off and the pragma below), atomics are integer atomics, every loop ends at
// a number the host passed or a device count clamped to it.
#pragma once
#include "evrep_common.h"
#include "evrep_ranksort.h"

// (At file scope the pragma also covers whatever the translation unit includes behind this file.  That changes nothing: the
// whole library is compiled with -ffp-contract=off, and the detector files behind it in evrep_capi_detin.hip repeat the same
// pragma for themselves.  It is here so that this file's rounding does not hang on a build flag.)
#pragma clang fp contract(off)

namespace evrep {

constexpr int kApSortTile = EVREP_AP_SORT_TILE;     // rows of a radix tile (one workgroup of 256 lanes, 8 rounds)
constexpr int kApScanTile = EVREP_AP_SCAN_TILE;     // rows of a scan tile (one wave, 8 rounds)
static_assert(EVREP_AP_GATHER_CHUNK == kDistThreads && EVREP_AP_GATHER_IMAGES == kThreads, "the gather's rounds are a workgroup wide");
constexpr int kApMaxT = EVREP_DETEVAL_MAX_T;
constexpr int kApPx = 1000, kApX = 101;
constexpr int kApBins = EVREP_NMS_MAX_CLASSES + 1;  // the classes and the bin of the rows that take part in nothing
static_assert(kApSortTile % kThreads == 0 && kApScanTile % kWave == 0, "whole rounds");

struct ApArgs {
    const uint8_t *tp;            // (n, T)
    const float *conf;            // (n)
    const float *pcls;            // (n)
    const float *tcls;            // (m)
    const int64_t *counts_dev;    // null, or {n, m} on the device (clamped to the capacities below)
    const double *tables;         // px[1000], x[101], d[100]
    double *p, *r, *f1, *ap;      // (nc, 1000) x 3, (nc, T)
    int64_t *n_labels, *n_pred;   // (nc)
    uint32_t *any_correct, *status;
    unsigned long long *key_a, *key_b;
    uint32_t *idx_a, *idx_b;
    uint32_t *hist;               // (256, sort tiles)
    uint32_t *cnt_p, *cnt_l;      // (nc + 1)
    uint32_t *seg;                // (nc + 2)
    float *sconf;                 // (n): the confidences in sorted order
    uint32_t *cum;                // (n, T)
    double *mpre;                 // (n, T)
    uint32_t *tsum;               // (scan tiles, T): sums, then exclusive bases
    double *thead, *tcarry;       // (scan tiles, T)
    uint32_t *tcls_head, *tcls_tail;   // (scan tiles)
    int64_t n, m;                 // capacities
    int32_t T, nc;
};

__device__ inline int64_t ap_rows(const ApArgs &a) {
    if (!a.counts_dev) return a.n;
    const int64_t v = a.counts_dev[0];
    return v < 0 ? 0 : (v > a.n ? a.n : v);
}
__device__ inline int64_t ap_targets(const ApArgs &a) {
    if (!a.counts_dev) return a.m;
    const int64_t v = a.counts_dev[1];
    return v < 0 ? 0 : (v > a.m ? a.m : v);
}

// int(c) when c is an integer in [0, nc), else nc (a NaN fails the comparisons)
__device__ inline uint32_t ap_class(float c, int nc) {
    return (c >= 0.0f && c < (float)nc && c == floorf(c)) ? (uint32_t)(int)c : (uint32_t)nc;
}

// ------------------------------------------------------------------------------------------------------------------ gather
struct ApGatherArgs {
    const uint8_t *correct;       // (B, max_det, T)
    const float *conf_cls;        // (B, max_det, 2)
    const int32_t *count;         // (B)
    const float *targets;         // (n_t, 2): image, class
    uint8_t *tp;                  // (cap_n, T)
    float *conf, *pcls;           // (cap_n)
    float *tcls;                  // (cap_m)
    int64_t *cursor;              // {rows so far, targets so far}
    int64_t n_t, cap_n, cap_m;
    int32_t B, max_det, T;
};

__device__ inline uint32_t ap_clamped_count(const ApGatherArgs &a, int b) {
    const int32_t c = a.count[b];
    return (uint32_t)(c < 0 ? 0 : (c > a.max_det ? a.max_det : c));
}

// grid (B), 256 threads
__global__ __launch_bounds__(kThreads) void k_ap_gather_rows(const ApGatherArgs a) {
    __shared__ uint32_t s_scan[kWaves];
    const int tid = threadIdx.x, b = blockIdx.x;
    uint32_t mine = 0;
    for (int i = tid; i < b; i += kThreads) mine += ap_clamped_count(a, i);
    uint32_t before;
    block_exclusive_scan<kWaves>(mine, s_scan, &before);
    const int64_t off = a.cursor[0] + (int64_t)before;
    const uint32_t cnt = ap_clamped_count(a, b);
    if (off < 0 || off + (int64_t)cnt > a.cap_n) return;               // (the caller sized the rows for every batch)
    const uint8_t *src = a.correct + (size_t)b * (size_t)a.max_det * (size_t)a.T;
    uint8_t *dst = a.tp + (size_t)off * (size_t)a.T;
    const uint32_t bytes = cnt * (uint32_t)a.T;
    for (uint32_t i = tid; i < bytes; i += kThreads) dst[i] = src[i];
    const float *cc = a.conf_cls + (size_t)b * (size_t)a.max_det * 2u;
    for (uint32_t i = tid; i < cnt; i += kThreads) {
        a.conf[off + i] = cc[2u * i];
        a.pcls[off + i] = cc[2u * i + 1u];
    }
}

// grid (1), 1024 threads
__global__ __launch_bounds__(kDistThreads) void k_ap_gather_finish(const ApGatherArgs a) {
    __shared__ uint32_t s_scan[kDistWaves];
    const int tid = threadIdx.x;
    const int64_t at = a.cursor[1];
    const float fB = (float)a.B;
    int64_t kept = 0;
    for (int64_t r0 = 0; r0 < a.n_t; r0 += kDistThreads) {
        const int64_t r = r0 + tid;
        const bool in = r < a.n_t;
        const float t0 = in ? a.targets[2 * r] : -1.0f;
        const bool keep = in && t0 >= 0.0f && t0 < fB && t0 == floorf(t0);
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<kDistWaves>(keep ? 1u : 0u, s_scan, &tot);
        const int64_t pos = at + kept + (int64_t)ex;
        if (keep && pos >= 0 && pos < a.cap_m) a.tcls[pos] = a.targets[2 * r + 1];
        kept += tot;
    }
    uint32_t mine = 0;
    for (int i = tid; i < a.B; i += kDistThreads) mine += ap_clamped_count(a, i);
    uint32_t rows;
    block_exclusive_scan<kDistWaves>(mine, s_scan, &rows);
    if (tid == 0) {
        a.cursor[0] += (int64_t)rows;
        a.cursor[1] = at + kept;
    }
}

// -------------------------------------------------------------------------------------------------------- keys and classes
// counts the classes `cls_at(i)` of i in [0, n) into cnt[0 .. nc]: an LDS histogram per workgroup, integer atomics behind it
template <class ClsAt>
__device__ inline void ap_count_classes(ClsAt cls_at, int64_t n, int nc, uint32_t *cnt, uint32_t *s_cnt) {
    for (int i = threadIdx.x; i <= nc; i += kThreads) s_cnt[i] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
        atomicAdd(&s_cnt[cls_at(i)], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i <= nc; i += kThreads)
        if (s_cnt[i]) atomicAdd(&cnt[i], s_cnt[i]);
}

// grid (<= 1024), 256 threads
__global__ __launch_bounds__(kThreads) void k_ap_keys(const ApArgs a) {
    __shared__ uint32_t s_cnt[kApBins];
    const int64_t n = ap_rows(a);
    uint32_t st = 0u;
    ap_count_classes([&](int64_t i) {
        const float cf = a.conf[i];
        const uint32_t c = ap_class(a.pcls[i], a.nc);
        if (c == (uint32_t)a.nc) st |= EVREP_AP_ST_BAD_CLASS;
        if (!(cf == cf)) st |= EVREP_AP_ST_NAN_CONF;
        a.key_a[i] = ((unsigned long long)c << 32) | (unsigned long long)(~rank_key(cf));
        a.idx_a[i] = (uint32_t)i;
        return c;
    }, n, a.nc, a.cnt_p, s_cnt);
    if (st) atomicOr(a.status, st);
}

// grid (<= 1024), 256 threads
__global__ __launch_bounds__(kThreads) void k_ap_targets(const ApArgs a) {
    __shared__ uint32_t s_cnt[kApBins];
    const int64_t m = ap_targets(a);
    uint32_t st = 0u;
    ap_count_classes([&](int64_t i) {
        const uint32_t c = ap_class(a.tcls[i], a.nc);
        if (c == (uint32_t)a.nc) st |= EVREP_AP_ST_BAD_CLASS;
        return c;
    }, m, a.nc, a.cnt_l, s_cnt);
    if (st) atomicOr(a.status, st);
}

// grid (1), 1024 threads: seg[c] = the sorted position of class c's first row, c in [0, nc + 1]; the two counts as int64
__global__ __launch_bounds__(kDistThreads) void k_ap_segments(const ApArgs a) {
    __shared__ uint32_t s_scan[kDistWaves];
    const int tid = threadIdx.x;
    uint32_t carry = 0;
    for (int c0 = 0; c0 <= a.nc; c0 += kDistThreads) {
        const int c = c0 + tid;
        const uint32_t v = c <= a.nc ? a.cnt_p[c] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<kDistWaves>(v, s_scan, &tot);
        if (c <= a.nc) a.seg[c] = carry + ex;
        if (c < a.nc) {
            a.n_pred[c] = (int64_t)v;
            a.n_labels[c] = (int64_t)a.cnt_l[c];
        }
        carry += tot;
    }
    if (tid == 0) a.seg[a.nc + 1] = carry;
}

// ---------------------------------------------------------------------------------------------------------------- the sort
struct ApSortArgs {
    const unsigned long long *key_in;
    const uint32_t *idx_in;
    unsigned long long *key_out;
    uint32_t *idx_out;
    uint32_t *hist;               // [digit * tiles + tile]
    int32_t shift, tiles;
};

// grid (tiles), 256 threads
__global__ __launch_bounds__(kThreads) void k_ap_radix_count(const ApArgs a, const ApSortArgs s) {
    __shared__ uint32_t s_hist[256];
    const int tid = threadIdx.x;
    const int64_t n = ap_rows(a), t0 = (int64_t)blockIdx.x * kApSortTile;
    s_hist[tid] = 0u;
    __syncthreads();
    for (int r = 0; r < kApSortTile / kThreads; ++r) {
        const int64_t i = t0 + r * kThreads + tid;
        if (i < n) atomicAdd(&s_hist[(uint32_t)(s.key_in[i] >> s.shift) & 255u], 1u);
    }
    __syncthreads();
    s.hist[(size_t)tid * (size_t)s.tiles + blockIdx.x] = s_hist[tid];
}

// grid (1), 1024 threads: the exclusive scan of hist in (digit, tile) order, in place
__global__ __launch_bounds__(kDistThreads) void k_ap_radix_scan(const ApSortArgs s) {
    __shared__ uint32_t s_scan[kDistWaves];
    const int tid = threadIdx.x;
    const int64_t total = 256 * (int64_t)s.tiles;
    uint32_t carry = 0;
    for (int64_t e0 = 0; e0 < total; e0 += kDistThreads) {
        const int64_t e = e0 + tid;
        const uint32_t v = e < total ? s.hist[e] : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<kDistWaves>(v, s_scan, &tot);
        if (e < total) s.hist[e] = carry + ex;
        carry += tot;
    }
}

// grid (tiles), 256 threads
__global__ __launch_bounds__(kThreads) void k_ap_radix_scatter(const ApArgs a, const ApSortArgs s) {
    __shared__ uint32_t s_base[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n = ap_rows(a), t0 = (int64_t)blockIdx.x * kApSortTile;
    s_base[tid] = s.hist[(size_t)tid * (size_t)s.tiles + blockIdx.x];
    __syncthreads();
    for (int r = 0; r < kApSortTile / kThreads; ++r) {
        const int64_t i = t0 + r * kThreads + tid;
        const bool valid = i < n;
        const unsigned long long key = valid ? s.key_in[i] : 0ull;
        const uint32_t row = valid ? s.idx_in[i] : 0u;
        const uint32_t digit = (uint32_t)(key >> s.shift) & 255u;
        uint32_t rank;
        bool last;
        wave_match(digit, 8, valid, lane, rank, last);
        for (int w = 0; w < kWaves; ++w) {                              // wave after wave: array order among equal digits
            if (wave == w && valid) {
                const uint32_t pos = s_base[digit] + rank;
                if ((int64_t)pos < n) {                                 // (holds by construction: the bases sum to n)
                    s.key_out[pos] = key;
                    s.idx_out[pos] = row;
                }
            }
            __syncthreads();
            if (wave == w && valid && last) s_base[digit] += rank + 1u;
            __syncthreads();
        }
    }
}

// grid (ceil(n / 256)), 256 threads
__global__ __launch_bounds__(kThreads) void k_ap_sorted_conf(const ApArgs a, const uint32_t *idx) {
    const int64_t n = ap_rows(a), i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) {
        const uint32_t row = idx[i];
        a.sconf[i] = (int64_t)row < n ? a.conf[row] : 0.0f;
    }
}

// --------------------------------------------------------------------------------------------------------------- the counts
// the sorted row i's tp bytes: tp + row * T
__device__ inline const uint8_t *ap_tp_row(const ApArgs &a, const uint32_t *idx, int64_t i, int64_t n) {
    const uint32_t row = idx[i];
    return a.tp + (size_t)((int64_t)row < n ? row : 0u) * (size_t)a.T;
}

// grid (ceil(scan tiles / 4)), 256 threads: a wave per tile.  WRITE false: the tile's sums; true: cum behind the tile's base
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_ap_cum(const ApArgs a, const uint32_t *idx) {
    const int lane = threadIdx.x & 63, T = a.T;
    const int64_t n = ap_rows(a), tile = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), t0 = tile * kApScanTile;
    if (t0 >= n) return;
    uint32_t run[kApMaxT];
#pragma unroll
    for (int j = 0; j < kApMaxT; ++j) run[j] = (WRITE && j < T) ? a.tsum[(size_t)tile * T + j] : 0u;
    const unsigned long long upto = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
    for (int r = 0; r < kApScanTile / kWave; ++r) {
        const int64_t i = t0 + r * kWave + lane;
        if (t0 + r * kWave >= n) break;                                 // (wave-uniform)
        const bool valid = i < n;
        const uint8_t *row = valid ? ap_tp_row(a, idx, i, n) : a.tp;
#pragma unroll
        for (int j = 0; j < kApMaxT; ++j) {
            if (j < T) {
                const unsigned long long bal = __ballot(valid && row[j] != 0);
                if (WRITE && valid) a.cum[(size_t)i * T + j] = run[j] + (uint32_t)__popcll(bal & upto);
                run[j] += (uint32_t)__popcll(bal);
            }
        }
    }
    if (!WRITE && lane == 0) {
#pragma unroll
        for (int j = 0; j < kApMaxT; ++j)
            if (j < T) a.tsum[(size_t)tile * T + j] = run[j];
    }
}

// grid (1), 64 threads: lane j turns the tiles' sums of threshold j into exclusive bases; any_correct
__global__ __launch_bounds__(kWave) void k_ap_cum_scan(const ApArgs a) {
    const int j = threadIdx.x;
    const int64_t n = ap_rows(a), tiles = (n + kApScanTile - 1) / kApScanTile;
    uint32_t carry = 0;
    if (j < a.T) {
        for (int64_t t = 0; t < tiles; ++t) {
            const uint32_t v = a.tsum[(size_t)t * a.T + j];
            a.tsum[(size_t)t * a.T + j] = carry;
            carry += v;
        }
    }
    const unsigned long long any = __ballot(carry != 0u);
    if (j == 0) *a.any_correct = any ? 1u : 0u;
}

// the count of true tp[., j] among the class's rows up to sorted row i; `first` = the class's first sorted row
__device__ inline uint32_t ap_tpc(const ApArgs &a, int64_t i, uint32_t first, int j) {
    const uint32_t base = first ? a.cum[(size_t)(first - 1u) * a.T + j] : 0u;
    return a.cum[(size_t)i * a.T + j] - base;
}

// ------------------------------------------------------------------------------------------------------------------- mpre
// grid (ceil(scan tiles / 4)), 256 threads: a wave per tile, from its last row to its first.  WRITE false: the maximum over
// the rows of the first row's class (thead) and the two boundary classes; true: mpre, with the carry of the tiles behind
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void k_ap_max(const ApArgs a, const unsigned long long *key) {
    const int lane = threadIdx.x & 63, T = a.T;
    const int64_t n = ap_rows(a), tile = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), t0 = tile * kApScanTile;
    if (t0 >= n) return;
    const int64_t t1 = t0 + kApScanTile < n ? t0 + kApScanTile : n;   // one past the tile's last row
    const uint32_t tail = (uint32_t)(key[t1 - 1] >> 32);
    uint32_t carry_cls = tail;
    double carry[kApMaxT];
#pragma unroll
    for (int j = 0; j < kApMaxT; ++j) carry[j] = (WRITE && j < T) ? a.tcarry[(size_t)tile * T + j] : 0.0;
    for (int r = kApScanTile / kWave - 1; r >= 0; --r) {
        if (t0 + r * kWave >= t1) continue;                             // (wave-uniform)
        const int64_t i = t0 + r * kWave + lane;
        const bool valid = i < t1;
        const uint32_t cls = valid ? (uint32_t)(key[i] >> 32) : 0xFFFFFFFFu;
        const uint32_t first = valid ? a.seg[cls <= (uint32_t)a.nc ? cls : (uint32_t)a.nc] : 0u;
        const double k = (double)(valid ? (i - (int64_t)first) + 1 : 1);
#pragma unroll
        for (int j = 0; j < kApMaxT; ++j) {
            if (j < T) {
                double v = valid ? (double)ap_tpc(a, i, first, j) / k : 0.0;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const double ov = __shfl_down(v, d, 64);
                    const uint32_t oc = __shfl_down(cls, d, 64);
                    if (lane + d < 64 && oc == cls && ov > v) v = ov;
                }
                if (cls == carry_cls && carry[j] > v) v = carry[j];
                if (WRITE && valid) a.mpre[(size_t)i * T + j] = v;
                carry[j] = __shfl(v, 0, 64);                             // lane 0 is valid: the round starts inside the tile
            }
        }
        carry_cls = __shfl(cls, 0, 64);
    }
    if (!WRITE && lane == 0) {
        a.tcls_head[tile] = carry_cls;
        a.tcls_tail[tile] = tail;
#pragma unroll
        for (int j = 0; j < kApMaxT; ++j)
            if (j < T) a.thead[(size_t)tile * T + j] = carry[j];
    }
}

// grid (1), 64 threads: lane j walks the tiles from the last; tcarry[t] = what the tiles behind t hand to its last class
__global__ __launch_bounds__(kWave) void k_ap_max_carry(const ApArgs a) {
    const int j = threadIdx.x;
    const int64_t n = ap_rows(a), tiles = (n + kApScanTile - 1) / kApScanTile;
    if (j >= a.T) return;
    double out = 0.0;
    uint32_t next_head = 0xFFFFFFFFu;
    for (int64_t t = tiles - 1; t >= 0; --t) {
        const uint32_t head = a.tcls_head[t], tail = a.tcls_tail[t];
        const double in = next_head == tail ? out : 0.0;
        a.tcarry[(size_t)t * a.T + j] = in;
        out = a.thead[(size_t)t * a.T + j];
        if (head == tail && in > out) out = in;
        next_head = head;
    }
}

// ----------------------------------------------------------------------------------------------------------------- curves
// A5 over the class's rows [first, first + np): x = -px, xp = -conf (float64), fp(k) given by the functor
template <class Fp>
__device__ inline double ap_interp_conf(const float *sconf, uint32_t first, uint32_t np, double px, double left, Fp fp) {
    const double x = -px;
    if (x < -(double)sconf[first]) return left;
    if (x > -(double)sconf[first + np - 1u]) return fp(np - 1u);
    uint32_t lo = 0u, hi = np - 1u;                                     // the largest k with xp[k] <= x
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (-(double)sconf[first + mid] <= x) lo = mid; else hi = mid - 1u;
    }
    if (lo == np - 1u) return fp(np - 1u);
    const double x0 = -(double)sconf[first + lo];
    if (x0 == x) return fp(lo);
    const double f0 = fp(lo), slope = (fp(lo + 1u) - f0) / (-(double)sconf[first + lo + 1u] - x0);
    return slope * (x - x0) + f0;
}

// grid (ceil(1000 / 256), nc), 256 threads
__global__ __launch_bounds__(kThreads) void k_ap_curves(const ApArgs a) {
    const int c = blockIdx.y, q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= kApPx) return;
    const uint32_t first = a.seg[c], np = a.seg[c + 1] - first, nl = a.cnt_l[c];
    if (np == 0u || nl == 0u) return;                                   // (the outputs were zeroed)
    const double px = a.tables[q], dl = (double)nl;
    const double r = ap_interp_conf(a.sconf, first, np, px, 0.0, [&](uint32_t k) { return (double)ap_tpc(a, (int64_t)first + k, first, 0) / dl; });
    const double p = ap_interp_conf(a.sconf, first, np, px, 1.0, [&](uint32_t k) { return (double)ap_tpc(a, (int64_t)first + k, first, 0) / (double)(k + 1u); });
    const size_t o = (size_t)c * kApPx + q;
    a.r[o] = r;
    a.p[o] = p;
    a.f1[o] = ((2.0 * p) * r) / ((p + r) + 1e-16);
}

// grid (ceil(nc * T / 4)), 256 threads: a wave per (class, threshold)
__global__ __launch_bounds__(kThreads) void k_ap_area(const ApArgs a) {
    __shared__ double s_y[kWaves][kApX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, T = a.T;
    const int64_t item = (int64_t)blockIdx.x * kWaves + wave;
    if (item >= (int64_t)a.nc * T) return;                              // (no barrier below: a wave works alone)
    const int c = (int)(item / T), j = (int)(item % T);
    const uint32_t first = a.seg[c], np = a.seg[c + 1] - first, nl = a.cnt_l[c];
    if (np == 0u || nl == 0u) return;
    const double dl = (double)nl;
    const int64_t L = (int64_t)np + 2;
    const double rlast = (double)ap_tpc(a, (int64_t)first + np - 1, first, j) / dl;
    const auto mrec = [&](int64_t k) -> double {
        if (k == 0) return 0.0;
        if (k == L - 1) return rlast + 0.01;
        return (double)ap_tpc(a, (int64_t)first + k - 1, first, j) / dl;
    };
    const auto mpre = [&](int64_t k) -> double {
        if (k == 0) return 1.0;                                         // max(1, every precision): a precision is <= 1
        if (k == L - 1) return 0.0;
        return a.mpre[(size_t)((int64_t)first + k - 1) * T + j];
    };
    const double *xs = a.tables + kApPx, *ds = xs + kApX;
    for (int i = lane; i < kApX; i += kWave) {
        const double x = xs[i];
        double y;
        if (x < 0.0) y = 1.0;                                           // (x < mrec[0]: left = mpre[0]; linspace has none)
        else if (x > mrec(L - 1)) y = 0.0;
        else {
            int64_t lo = 0, hi = L - 1;                                 // the largest k with mrec[k] <= x
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo + 1) / 2;
                if (mrec(mid) <= x) lo = mid; else hi = mid - 1;
            }
            const double x0 = mrec(lo);
            if (lo == L - 1) y = 0.0;
            else if (x0 == x) y = mpre(lo);
            else {
                const double f0 = mpre(lo), slope = (mpre(lo + 1) - f0) / (mrec(lo + 1) - x0);
                y = slope * (x - x0) + f0;
            }
        }
        s_y[wave][i] = y;
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    if (lane == 0) {
        double sum = 0.0;
        for (int i = 0; i < kApX - 1; ++i) sum = sum + (ds[i] * (s_y[wave][i] + s_y[wave][i + 1])) / 2.0;
        a.ap[(size_t)c * T + j] = sum;
    }
}

}  // namespace evrep
