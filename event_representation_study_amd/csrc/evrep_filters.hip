// evrep_filters.hip -- the ev-licious event filters (ev-licious/src/evlicious/tools/filters.py, tools/utils.py) on the device:
// RefractoryPeriod, ContrastThresholdIncrease, the change map of resize_to_resolution, BackgroundActivity, the HotPixel mask
// gather, and the stable compaction of the kept rows.  Every filter writes one keep byte per event in ARRAY order and carries
// the reference's per-pixel state array in and out, so successive windows of one recording chain calls.
//
// The per-pixel state machines walk the PIXEL-SORTED stream of the binning pass (sorted2: ordered by window, pixel id, rank;
// chunk_off: where every (row, 128-pixel chunk) starts): a pixel's records lie side by side in array order, which is all a
// sequential per-pixel recurrence needs.  One lane per record; the lane that holds the FIRST record of a pixel walks the
// pixel's whole list.  Sparse windows (about one record per pixel) keep every lane busy; a hot pixel of n records is one
// lane walking n records while its wave waits -- the accepted bound (NOTES.md).
#pragma once
#include "evrep_common.h"

namespace evrep {

constexpr int kFiltThreads = 256;

// ---- the state machines: S = the reference's state array element, step() = one iteration of its loop for one pixel ----
// RefractoryPeriod (utils.py:193-200): `if t[i] - last[y, x] < period: drop` else last = t.  float64 state, -inf at rest.
struct FsmRefractory {
    using S = double;
    double period;
    __device__ bool step(S &s, const Rec &r, int64_t tb) const {
        const double t = (double)(tb + (int64_t)r.z);
        if (t - s < period) return false;
        s = t;
        return true;
    }
};
// ContrastThresholdIncrease (utils.py:184-191): activity += p; |activity| >= factor: pass and reset.  int32 state.
struct FsmContrast {
    using S = int32_t;
    double factor;
    __device__ bool step(S &s, const Rec &r, int64_t) const {
        s += r.w;
        if (fabs((double)s) >= factor) { s = 0; return true; }
        return false;
    }
};
// resize_to_resolution's change map (utils.py:143-158) on a batch whose coordinates are CELLS: change += p * 1.0 / (fx * fy)
// -- the sum formed in float64 and rounded to float32 by the store -- ; |change| >= 1: pass, change -= p.  float32 state.
struct FsmChangeMap {
    using S = float;
    double cells;
    __device__ bool step(S &s, const Rec &r, int64_t) const {
        const double p = (double)r.w;
        s = (float)((double)s + p / cells);
        if (fabsf(s) >= 1.0f) { s = (float)((double)s - p); return true; }
        return false;
    }
};

// grid (ceil(max_events_per_window / 256), B), 256 threads.  sorted / chunk_off: the pixel-sorted stream.  state [B][H*W] in/out,
// keep [total] (cleared by the caller: out-of-frame events, which the stream does not hold, stay dropped).
// The binning pass keys a record by x + y * W and drops the keys outside [0, H * W): an event with y outside the frame never
// reaches the stream, but one with x outside [0, W) and a key inside lands in a NEIGHBOUR row's pixel.  Only windows whose
// bounding box (WindowMeta, all events, raw coordinates) leaves the frame in x can hold such records; there every record is
// checked against its event row (the record's rank) and skipped, so an out-of-frame event is dropped and touches no state.
__device__ inline bool x_aliases(const WindowMeta &m, int W) { return m.xmin < 0 || m.xmax >= W; }

template <typename F>
__global__ __launch_bounds__(kFiltThreads) void k_filter_pixel_fsm(const Rec *__restrict__ sorted, const uint32_t *__restrict__ chunk_off,
                                                                  const int64_t *__restrict__ off, const int64_t *__restrict__ t_base,
                                                                  const int4 *__restrict__ ev, const WindowMeta *__restrict__ meta,
                                                                  int H, int W, int nchunk, F f, typename F::S *__restrict__ state,
                                                                  uint8_t *__restrict__ keep) {
    const int b = blockIdx.y;
    const int64_t beg = off[b];
    const uint32_t n_win = (uint32_t)(off[b + 1] - beg);
    // the window's in-frame records: [beg, end of its last row)
    const uint32_t lo = (uint32_t)beg, hi = chunk_off[((size_t)b * H + (H - 1)) * (nchunk + 1) + nchunk];
    const uint32_t j = lo + blockIdx.x * kFiltThreads + threadIdx.x;
    if (j >= hi || hi - lo > n_win) return;
    Rec r = sorted[j];
    const int pix = r.x;
    if (j > lo && sorted[j - 1].x == pix) return;   // not the first record of its pixel
    if ((uint32_t)pix >= (uint32_t)(H * W)) return;
    const int64_t tb = t_base ? t_base[b] : 0;
    const int4 *evw = x_aliases(meta[b], W) ? ev + beg : nullptr;
    typename F::S *sp = state + (size_t)b * H * W + pix;
    typename F::S s = *sp;
    uint32_t at = j;
    for (;;) {
        if ((uint32_t)r.y < n_win && (!evw || (uint32_t)evw[r.y].x < (uint32_t)W)) keep[beg + r.y] = f.step(s, r, tb) ? 1 : 0;
        if (++at >= hi) break;
        r = sorted[at];
        if (r.x != pix) break;
    }
    *sp = s;
}

// ---- BackgroundActivity (utils.py:170-179) ----
// Every event, kept or not, writes its t into rows [max(y - r, 0), y + r), columns [max(x - r, 0), x + r) of `timestamps`, so the
// value event i reads at its own pixel is the t of the LATEST EARLIER event j (array order) with x_i - r + 1 <= x_j <= x_i + r and
// y_i - r + 1 <= y_j <= y_i + r, else the incoming state: no sequential dependence.  ba_latest finds that record: per neighbour
// row the <= 2r neighbour pixels are one contiguous stretch of the stream; inside it, pixel by pixel, a binary search for the
// largest rank below `rank_lim`.  Returns the rank (-1: none) and the record's t.
__device__ inline int ba_latest(const Rec *__restrict__ sorted, const uint32_t *__restrict__ chunk_off, int b, int H, int W, int nchunk,
                                int x, int y, int radius, int rank_lim, const int4 *__restrict__ evw, int &t_out) {
    int best = -1;
    const int y0 = max(y - radius + 1, 0), y1 = min(y + radius, H - 1);
    const int x0 = max(x - radius + 1, 0), x1 = min(x + radius, W - 1);
    if (x0 > x1) return best;
    for (int ny = y0; ny <= y1; ++ny) {
        const uint32_t *co = chunk_off + ((size_t)b * H + ny) * (nchunk + 1);
        uint32_t lo = co[x0 / kChunkPx];
        const uint32_t end = co[x1 / kChunkPx + 1];
        const int key0 = ny * W + x0, key1 = ny * W + x1;
        uint32_t hi = end;
        while (lo < hi) {   // first record with pixel id >= key0
            const uint32_t mid = (lo + hi) >> 1;
            if (sorted[mid].x < key0) lo = mid + 1; else hi = mid;
        }
        uint32_t pos = lo;
        while (pos < end) {
            const int pix = sorted[pos].x;
            if (pix > key1) break;
            uint32_t a = pos + 1, q = end;   // q = first record behind this pixel's run
            while (a < q) {
                const uint32_t mid = (a + q) >> 1;
                if (sorted[mid].x <= pix) a = mid + 1; else q = mid;
            }
            uint32_t c = pos, d = q;         // c = first record of the run with rank >= rank_lim
            while (c < d) {
                const uint32_t mid = (c + d) >> 1;
                if (sorted[mid].y < rank_lim) c = mid + 1; else d = mid;
            }
            for (uint32_t k = c; k > pos; --k) {   // evw (see x_aliases): step back over the records of out-of-frame events
                const Rec e = sorted[k - 1];
                if (evw && (uint32_t)evw[e.y].x >= (uint32_t)W) continue;
                if (e.y > best) { best = e.y; t_out = e.z; }
                break;
            }
            pos = q;
        }
    }
    return best;
}

// grid (ceil(max_events_per_window / 256), B), 256 threads: one lane per event, array order.  state is only read.
__global__ __launch_bounds__(kFiltThreads) void k_filter_background(const int4 *__restrict__ ev, const Rec *__restrict__ sorted,
                                                                   const uint32_t *__restrict__ chunk_off, const int64_t *__restrict__ off,
                                                                   const int64_t *__restrict__ t_base, const WindowMeta *__restrict__ meta,
                                                                   int H, int W, int nchunk, double depth, int radius,
                                                                   const double *__restrict__ state,
                                                                   uint8_t *__restrict__ keep) {
    const int b = blockIdx.y;
    const int64_t beg = off[b];
    const int64_t n_win = off[b + 1] - beg;
    const int64_t i = (int64_t)blockIdx.x * kFiltThreads + threadIdx.x;
    if (i >= n_win) return;
    const int4 e = ev[beg + i];
    if ((uint32_t)e.x >= (uint32_t)W || (uint32_t)e.y >= (uint32_t)H) { keep[beg + i] = 0; return; }
    const int64_t tb = t_base ? t_base[b] : 0;
    int tj = 0;
    const int rk = ba_latest(sorted, chunk_off, b, H, W, nchunk, e.x, e.y, radius, (int)i, x_aliases(meta[b], W) ? ev + beg : nullptr, tj);
    const double t_last = rk >= 0 ? (double)(tb + (int64_t)tj) : state[(size_t)b * H * W + (size_t)e.y * W + e.x];
    const double t = (double)(tb + (int64_t)e.z);
    const bool discard = t_last > 0.0 && t - t_last > depth;
    keep[beg + i] = discard ? 0 : 1;
}

// grid (ceil(H * W / 256), B), 256 threads: the outgoing `timestamps` array -- a pixel holds the t of the last event that wrote it.
// Runs behind k_filter_background on the same stream (that kernel reads the incoming values).
__global__ __launch_bounds__(kFiltThreads) void k_filter_background_state(const Rec *__restrict__ sorted, const uint32_t *__restrict__ chunk_off,
                                                                         const int64_t *__restrict__ off, const int64_t *__restrict__ t_base,
                                                                         const int4 *__restrict__ ev, const WindowMeta *__restrict__ meta,
                                                                         int H, int W, int nchunk, int radius, double *__restrict__ state) {
    const int b = blockIdx.y;
    const int cell = blockIdx.x * kFiltThreads + threadIdx.x;
    if (cell >= H * W) return;
    const int y = cell / W, x = cell - y * W;
    int tj = 0;
    const int rk = ba_latest(sorted, chunk_off, b, H, W, nchunk, x, y, radius, INT32_MAX, x_aliases(meta[b], W) ? ev + off[b] : nullptr, tj);
    if (rk >= 0) state[(size_t)b * H * W + cell] = (double)((t_base ? t_base[b] : 0) + (int64_t)tj);
}

// ---- HotPixel: keep[i] = mask[b, y, x] (filters.py:53) ----
// grid (ceil(max_events_per_window / 256), B), 256 threads.
__global__ __launch_bounds__(kFiltThreads) void k_filter_mask_gather(const int4 *__restrict__ ev, const int64_t *__restrict__ off, int H, int W,
                                                                    const uint8_t *__restrict__ mask, uint8_t *__restrict__ keep) {
    const int b = blockIdx.y;
    const int64_t beg = off[b];
    const int64_t i = (int64_t)blockIdx.x * kFiltThreads + threadIdx.x;
    if (i >= off[b + 1] - beg) return;
    const int4 e = ev[beg + i];
    uint8_t k = 0;
    if ((uint32_t)e.x < (uint32_t)W && (uint32_t)e.y < (uint32_t)H) k = mask[(size_t)b * H * W + (size_t)e.y * W + e.x] ? 1 : 0;
    keep[beg + i] = k;
}

// ---- resize_to_resolution: (x, y) -> the cell (x // fx, y // fy) (utils.py:150-151) ----
// Multiply-shift reciprocals made on the host: floor(v / d) = mulhi(v, m) with m = floor(2^32 / d) + 1 (0 stands for d == 1),
// exact for v < 4096 = EVREP_MAX_DIM and d <= 4096 (the error v * 2^-32 stays below 1 / d).  Out-of-frame events get the
// coordinates (-1, -1): out of the coarse frame as well.
// grid (ceil(total / 256)), 256 threads.
__global__ __launch_bounds__(kFiltThreads) void k_filter_cell_map(const int4 *__restrict__ ev, int64_t total, int H, int W, uint32_t mx, uint32_t my,
                                                                 int4 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kFiltThreads + threadIdx.x;
    if (i >= total) return;
    int4 e = ev[i];
    const bool in = (uint32_t)e.x < (uint32_t)W && (uint32_t)e.y < (uint32_t)H;
    e.x = in ? (int)(mx ? __umulhi((uint32_t)e.x, mx) : (uint32_t)e.x) : -1;
    e.y = in ? (int)(my ? __umulhi((uint32_t)e.y, my) : (uint32_t)e.y) : -1;
    out[i] = e;
}

// ---- stable compaction of the kept rows of all windows ----
// The concatenated rows [offsets[0], offsets[B]) are cut into kCompactSlices contiguous slices, one workgroup each; a slice is
// walked in rounds of 1024 rows, in order, so the compaction is STABLE.  The slices meet through scratch (uint32 [kCompactSlices]
// counts, then their exclusive prefix in place).  Sizes are read on the device: nothing returns to the host.
constexpr int kCompactSlices = 1024;
constexpr int kCompactThreads = 1024;
__host__ __device__ inline size_t filter_compact_scratch_bytes() { return (size_t)(kCompactSlices + 1) * sizeof(uint32_t); }

__device__ inline void compact_slice(const int64_t *__restrict__ off, int B, int s, int64_t &lo, int64_t &hi) {
    const int64_t first = off[0], n = off[B] - first;
    const int64_t per = (n + kCompactSlices - 1) / kCompactSlices;
    lo = first + min((int64_t)s * per, n);
    hi = min(lo + per, first + n);
}

// grid (kCompactSlices), 1024 threads: WRITE = false counts the slice's kept rows, WRITE = true places them.
template <bool WRITE>
__global__ __launch_bounds__(kCompactThreads) void k_filter_compact(const int4 *__restrict__ ev, const int64_t *__restrict__ off, int B,
                                                                   const uint8_t *__restrict__ keep, uint32_t *__restrict__ scratch,
                                                                   int4 *__restrict__ out) {
    __shared__ uint32_t tmp[kCompactThreads / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    int64_t lo, hi;
    compact_slice(off, B, s, lo, hi);
    uint32_t base = WRITE ? scratch[s] : 0u;
    for (int64_t r0 = lo; r0 < hi; r0 += kCompactThreads) {   // uniform
        const int64_t i = r0 + tid;
        const uint32_t k = (i < hi && keep[i]) ? 1u : 0u;
        uint32_t tot;
        const uint32_t pre = block_exclusive_scan<kCompactThreads / 64>(k, tmp, &tot);
        if (WRITE && k) out[(size_t)base + pre] = ev[i];
        base += tot;
    }
    if (!WRITE && tid == 0) scratch[s] = base;
}

// grid (1), 1024 threads: the slice counts -> their exclusive prefix, in place; entry kCompactSlices = the kept total.
__global__ __launch_bounds__(kCompactThreads) void k_filter_compact_scan(uint32_t *__restrict__ scratch) {
    __shared__ uint32_t tmp[kCompactThreads / 64];
    static_assert(kCompactSlices == kCompactThreads, "one slice count per thread");
    const uint32_t v = scratch[threadIdx.x];
    uint32_t tot;
    const uint32_t pre = block_exclusive_scan<kCompactThreads / 64>(v, tmp, &tot);
    scratch[threadIdx.x] = pre;
    if (threadIdx.x == 0) scratch[kCompactSlices] = tot;
}

// grid (B + 1), 64 threads: offsets_out[b] = kept rows in front of window b = the prefix of the slice that holds offsets[b] + the
// kept rows of that slice in front of it.
__global__ __launch_bounds__(kWave) void k_filter_compact_offsets(const int64_t *__restrict__ off, int B, const uint8_t *__restrict__ keep,
                                                                 const uint32_t *__restrict__ scratch, int64_t *__restrict__ off_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t first = off[0], n = off[B] - first;
    const int64_t pos = min(max(off[b], first), first + n);
    if (b == B || n == 0) {
        if (lane == 0) off_out[b] = b == B ? (int64_t)scratch[kCompactSlices] : 0;
        return;
    }
    const int64_t per = (n + kCompactSlices - 1) / kCompactSlices;
    const int s = (int)min((pos - first) / per, (int64_t)kCompactSlices - 1);
    int64_t lo, hi;
    compact_slice(off, B, s, lo, hi);
    uint32_t c = 0;
    for (int64_t i = lo + lane; i < pos; i += kWave) c += keep[i] ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) off_out[b] = (int64_t)scratch[s] + c;
}

}  // namespace evrep
