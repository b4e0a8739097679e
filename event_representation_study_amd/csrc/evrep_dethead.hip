// evrep_dethead.hip -- what ev-YOLOv6's Detect.forward does behind its last convolutions (yolov6/models/effidehead.py:89-173
// with generate_anchors(is_eval=True) and dist2bbox(xywh) behind it): the per-level NCHW maps of cls_preds / reg_preds ->
// the prediction tensor (B, N, 5 + nc) in evaluation, (pred_scores, pred_distri) in training, and the gradients of the maps
// from the gradients of those two.  include/evrep.h states the rules with evrep_dethead_predict.
//
//   k_dethead_predict   grid (tiles, B): a workgroup owns a tile of kDetheadTile consecutive anchors of one (image, level).
//                       Wave s decodes side s, a lane per anchor: the lane's K logits go through LDS once (its own column, no
//                       bank shared with another lane) and dfl_side of evrep_dfl.h.  Wave 0 then forms the box rows; all four
//                       waves the class columns, a wave per class plane, a lane per anchor: the maps are read along h * w.
//   k_dethead_train     the same tile: sigmoid of the class planes into pred_scores' rows, the regression planes into
//                       pred_distri's rows, bit for bit.
//   k_dethead_backward  the tile in the other direction: the rows of grad_scores (times (1 - p) * p of the stored scores) and
//                       of grad_distri come in as one span, the planes of the maps' gradients go out a lane per anchor.
//
// THE TILE.  A row of the outputs is 5 + nc, nc or 4K floats, so a lane per anchor would store with that stride.  The tile's
// rows are staged in LDS instead -- row stride `ld` = the row's width rounded up to odd, so the 32 lanes of a half wave that
// write one column fall on 32 different banks whatever the width -- and leave as ONE contiguous span of global memory:
// 4-byte stores up to the first 16-byte boundary, 16 bytes per lane from there, 4-byte stores for the last 0..3 floats
// (span_store).  A row wider than kDetheadCols floats goes through in chunks of that many columns; a chunk that is not the
// whole row leaves as one span per anchor, a wave per row.
//
// ROUNDING.  Box and class columns: every statement ONE float64 operation (__dadd_rn ...), the maps' values widened exactly, one
// rounding to float32 at the store into the tile.  The backward is float32, one operation per statement (__fsub_rn / __fmul_rn).
// The library is compiled with -ffp-contract=off and this file repeats it as a pragma.
//
// THE MAPS' DTYPE.  The three kernels take the maps' element type as a template parameter (EVREP_DT_F32, _F16, _BF16: float, or
// the 16 bits of a float16 / bfloat16 as uint16_t).  Only planes_to_tile, the E1 logit loads and tile_to_planes touch the maps:
// a 16-bit element is widened exactly at the load (rule W1) and the backward's float32 value is rounded once at the store (W2),
// by the integer functions of evrep_f16.h.  A lane moves ONE element, 2 bytes: a wave's 64 anchors of a plane are 128
// contiguous bytes whatever the plane's start (planes of odd h * w start 2-byte aligned only), so there is no wide path whose
// first, last and odd-start elements would need a narrow twin.  The LDS tile, dfl_side and the float32 spans are as before.
//
// Every loop ends at a value the host passed and every index is below the size the host stated.  Plain C++ and vector stores,
// no atomic, no scratch, nothing read back, no allocation: the launches can be captured into a graph and two calls give equal
// bits.
#pragma once
#include "evrep_common.h"
#include "evrep_dfl.h"
#include "evrep_f16.h"

#pragma clang fp contract(off)

namespace evrep {

constexpr int kDetheadTile = EVREP_DETHEAD_TILE;                         // anchors of a tile: a lane each
constexpr int kDetheadCols = 4 * (EVREP_DETLOSS_MAX_REG + 1);            // columns of a chunk: the widest row of pred_distri
constexpr int kDetheadLds = kDetheadTile * (kDetheadCols | 1);           // floats of the staged tile
static_assert(kDetheadTile == kWave && kThreads == 4 * kWave, "a lane per anchor, a wave per side");
static_assert(kDetheadLds >= (EVREP_DETLOSS_MAX_REG + 1) * kThreads, "the sides' logits share the tile's LDS");

struct DetheadArgs {
    const void *cls[EVREP_DETHEAD_MAX_LEVELS];    // [B, nc, h, w] per level: logits (the forward), null in the backward
    const void *reg[EVREP_DETHEAD_MAX_LEVELS];    // [B, 4K, h, w]; the element type is the kernel's template parameter
    void *gcls[EVREP_DETHEAD_MAX_LEVELS];         // the backward's outputs, same shapes and element type
    void *greg[EVREP_DETHEAD_MAX_LEVELS];
    int32_t n[EVREP_DETHEAD_MAX_LEVELS];          // h * w
    int32_t w[EVREP_DETHEAD_MAX_LEVELS];
    int32_t off[EVREP_DETHEAD_MAX_LEVELS];        // the level's first anchor
    int32_t tile0[EVREP_DETHEAD_MAX_LEVELS];      // the level's first tile
    float stride[EVREP_DETHEAD_MAX_LEVELS];
    float *pred;                  // (B, N, 5 + nc)
    float *scores, *distri;       // (B, N, nc), (B, N, 4K)
    const float *p, *gs, *gd;     // the backward's inputs: stored scores, grad_scores, grad_distri
    int32_t L, N, nc, K, use_dfl;
};

// the tile of workgroup blockIdx.x: its level, first anchor inside the level and number of anchors (1..kDetheadTile)
__device__ inline void dethead_tile(const DetheadArgs &t, int &l, int &a0, int &cnt) {
    l = 0;
    for (int i = 1; i < t.L; ++i) l = (int)blockIdx.x >= t.tile0[i] ? i : l;
    a0 = ((int)blockIdx.x - t.tile0[l]) * kDetheadTile;
    const int left = t.n[l] - a0;
    cnt = left < kDetheadTile ? left : kDetheadTile;
}

// `n` floats to dst from the staged rows: float g of the span is column g % cw of row r0 + g / cw.  `nth` threads, this one `tid`.
__device__ inline void span_store(float *dst, int n, const float *tile, int ld, int cw, int r0, int tid, int nth) {
    const int mis = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3u);
    int head = (4 - mis) & 3;
    head = head < n ? head : n;
    const int nb = (n - head) >> 2;
    for (int g = tid; g < head; g += nth) gstore_f32(dst + g, tile[(size_t)(r0 + g / cw) * ld + g % cw]);
    for (int j = tid; j < nb; j += nth) {
        const int g = head + 4 * j;
        int r = g / cw, c = g - r * cw;
        uint32_t v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[q] = __float_as_uint(tile[(size_t)(r0 + r) * ld + c]);
            if (++c == cw) { c = 0; ++r; }
        }
        gstore16(dst + g, make_uint4(v[0], v[1], v[2], v[3]));
    }
    for (int g = head + 4 * nb + tid; g < n; g += nth) gstore_f32(dst + g, tile[(size_t)(r0 + g / cw) * ld + g % cw]);
}

// the staged columns [0, cw) of the tile's `cnt` rows -> columns [c0, c0 + cw) of the rows of `out` (row length `row`) that
// start at out_row0: one span when the chunk is the whole row, else a span per anchor.  All 256 threads call it.
__device__ inline void tile_store(float *out_row0, int row, int c0, int cw, int cnt, const float *tile, int ld) {
    if (cw == row) {
        span_store(out_row0, cnt * cw, tile, ld, cw, 0, (int)threadIdx.x, kThreads);
    } else {
        for (int r = (int)(threadIdx.x >> 6); r < cnt; r += kWaves)
            span_store(out_row0 + (size_t)r * row + c0, cw, tile, ld, cw, r, (int)(threadIdx.x & 63), kWave);
    }
}

// E4 / T1: the sigmoid of a logit, three float64 operations and one rounding
__device__ inline float dethead_sigmoid(float x) {
    const double e = exp(-(double)x);
    return (float)__ddiv_rn(1.0, __dadd_rn(1.0, e));
}

// a map's element: float, or the 16 bits of a float16 / bfloat16; W1 at the load, W2 at the store
template <int kDt> struct DetheadMap { typedef uint16_t elem; };
template <> struct DetheadMap<EVREP_DT_F32> { typedef float elem; };
template <int kDt> __device__ inline float dethead_widen(typename DetheadMap<kDt>::elem v) {
    if constexpr (kDt == EVREP_DT_F32) return v;
    else if constexpr (kDt == EVREP_DT_F16) return widen_f16(v);
    else return widen_bf16(v);
}
__device__ inline void gstore_u16(uint16_t *p, uint16_t v) {
    *reinterpret_cast<uint16_t __attribute__((address_space(1))) *>(reinterpret_cast<uintptr_t>(p)) = v;
}
template <int kDt> __device__ inline void dethead_store(typename DetheadMap<kDt>::elem *p, float v) {
    if constexpr (kDt == EVREP_DT_F32) gstore_f32(p, v);
    else if constexpr (kDt == EVREP_DT_F16) gstore_u16(p, round_f16(v));
    else gstore_u16(p, round_bf16(v));
}

// planes [ch0, ch0 + cw) of a level's map (of `chans` planes per image) -> the tile's columns [col0, col0 + cw): a wave per
// plane, a lane per anchor
template <bool kSigmoid, int kDt>
__device__ inline void planes_to_tile(const void *__restrict__ map, int b, int chans, int n, int a0, int cnt, int ch0, int cw,
                                      float *tile, int ld, int col0) {
    typedef typename DetheadMap<kDt>::elem E;
    const int lane = (int)(threadIdx.x & 63);
    if (lane >= cnt) return;
    const E *src = static_cast<const E *>(map) + ((size_t)b * chans + (size_t)ch0) * (size_t)n + (size_t)(a0 + lane);   // plane c: src[c * n]
    float *dst = tile + (size_t)lane * ld + col0;
    int c = (int)(threadIdx.x >> 6);
    for (; c + 3 * kWaves < cw; c += 4 * kWaves) {                       // four loads in flight per lane
        float x[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) x[q] = dethead_widen<kDt>(src[(size_t)(c + q * kWaves) * n]);
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[c + q * kWaves] = kSigmoid ? dethead_sigmoid(x[q]) : x[q];
    }
    for (; c < cw; c += kWaves) {
        const float x = dethead_widen<kDt>(src[(size_t)c * n]);
        dst[c] = kSigmoid ? dethead_sigmoid(x) : x;
    }
}

// ------------------------------------------------------------------------------------------------------------------- predict
template <int kDt>
__global__ __launch_bounds__(kThreads) void k_dethead_predict(const DetheadArgs t) {
    typedef typename DetheadMap<kDt>::elem E;
    __shared__ float tile[kDetheadLds];
    __shared__ double dist[4][kDetheadTile];
    int l, a0, cnt;
    dethead_tile(t, l, a0, cnt);
    const int b = blockIdx.y, n = t.n[l], row = 5 + t.nc;
    const int lane = (int)(threadIdx.x & 63), side = (int)(threadIdx.x >> 6);
    float *out_row0 = t.pred + ((size_t)b * t.N + (size_t)(t.off[l] + a0)) * (size_t)row;
    // E1: the lane's K logits, one read each, into its own column of LDS
    if (lane < cnt) {
        const E *z = static_cast<const E *>(t.reg[l]) + ((size_t)b * 4u * t.K + (size_t)side * t.K) * (size_t)n + (size_t)(a0 + lane);
        float *mine = tile + threadIdx.x;
        int k = 0;
        for (; k + 3 < t.K; k += 4) {                                    // four loads in flight per lane
            float x[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = dethead_widen<kDt>(z[(size_t)(k + q) * n]);
#pragma unroll
            for (int q = 0; q < 4; ++q) mine[(k + q) * kThreads] = x[q];
        }
        for (; k < t.K; ++k) mine[k * kThreads] = dethead_widen<kDt>(z[(size_t)k * n]);
        double m, Z, d;
        if (t.use_dfl) dfl_side(mine, kThreads, t.K, m, Z, d);
        else d = (double)mine[0];
        dist[side][lane] = d;
    }
    __syncthreads();                                                     // the logits are spent: the LDS becomes the tile
    for (int c0 = 0; c0 < row; c0 += kDetheadCols) {
        const int cw = row - c0 < kDetheadCols ? row - c0 : kDetheadCols, ld = cw | 1;
        int first = 0;                                                   // the chunk's first class column
        if (c0 == 0) {
            first = row < 5 ? row : 5;
            if (side == 0 && lane < cnt) {                               // E2, E3
                const int a = a0 + lane, i = a / t.w[l], j = a - i * t.w[l];
                const double ax = __dadd_rn((double)j, 0.5), ay = __dadd_rn((double)i, 0.5), s = (double)t.stride[l];
                const double x1 = __dsub_rn(ax, dist[0][lane]), y1 = __dsub_rn(ay, dist[1][lane]);
                const double x2 = __dadd_rn(ax, dist[2][lane]), y2 = __dadd_rn(ay, dist[3][lane]);
                const double cx = __ddiv_rn(__dadd_rn(x1, x2), 2.0), cy = __ddiv_rn(__dadd_rn(y1, y2), 2.0);
                const double bw = __dsub_rn(x2, x1), bh = __dsub_rn(y2, y1);
                float *r = tile + (size_t)lane * ld;
                r[0] = (float)__dmul_rn(cx, s);
                r[1] = (float)__dmul_rn(cy, s);
                r[2] = (float)__dmul_rn(bw, s);
                r[3] = (float)__dmul_rn(bh, s);
                r[4] = 1.0f;
            }
        }
        planes_to_tile<true, kDt>(t.cls[l], b, t.nc, n, a0, cnt, c0 + first - 5, cw - first, tile, ld, first);   // E4
        __syncthreads();
        tile_store(out_row0, row, c0, cw, cnt, tile, ld);
        __syncthreads();
    }
}

// --------------------------------------------------------------------------------------------------------------------- train
template <int kDt>
__global__ __launch_bounds__(kThreads) void k_dethead_train(const DetheadArgs t) {
    __shared__ float tile[kDetheadLds];
    int l, a0, cnt;
    dethead_tile(t, l, a0, cnt);
    const int b = blockIdx.y, n = t.n[l];
    const size_t at = (size_t)b * t.N + (size_t)(t.off[l] + a0);
    for (int c0 = 0; c0 < t.nc; c0 += kDetheadCols) {                    // T1
        const int cw = t.nc - c0 < kDetheadCols ? t.nc - c0 : kDetheadCols, ld = cw | 1;
        planes_to_tile<true, kDt>(t.cls[l], b, t.nc, n, a0, cnt, c0, cw, tile, ld, 0);
        __syncthreads();
        tile_store(t.scores + at * (size_t)t.nc, t.nc, c0, cw, cnt, tile, ld);
        __syncthreads();
    }
    const int row = 4 * t.K, ld = row | 1;                               // T2: row <= kDetheadCols, one chunk
    planes_to_tile<false, kDt>(t.reg[l], b, row, n, a0, cnt, 0, row, tile, ld, 0);
    __syncthreads();
    tile_store(t.distri + at * (size_t)row, row, 0, row, cnt, tile, ld);
}

// ------------------------------------------------------------------------------------------------------------------ backward
// `n` floats of src (times (1 - p) * p of `p` when given) into the staged rows, as span_store lays them out
__device__ inline void span_load(const float *__restrict__ src, const float *__restrict__ p, int n, float *tile, int ld, int cw,
                                 int r0, int tid, int nth) {
    const int mis = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3u);
    int head = (4 - mis) & 3;
    head = head < n ? head : n;
    const int nb = (n - head) >> 2;
    const auto one = [&](int g) {
        float v = src[g];
        if (p) { const float y = p[g]; v = __fmul_rn(__fmul_rn(v, __fsub_rn(1.0f, y)), y); }
        tile[(size_t)(r0 + g / cw) * ld + g % cw] = v;
    };
    for (int g = tid; g < head; g += nth) one(g);
    const bool p16 = p && ((reinterpret_cast<uintptr_t>(p) ^ reinterpret_cast<uintptr_t>(src)) & 15u) == 0u;
    for (int j = tid; j < nb; j += nth) {
        const int g = head + 4 * j;
        const float4 v4 = gload16f(src + g);
        float v[4] = {v4.x, v4.y, v4.z, v4.w};
        if (p) {
            float y[4];
            if (p16) { const float4 y4 = gload16f(p + g); y[0] = y4.x; y[1] = y4.y; y[2] = y4.z; y[3] = y4.w; }
            else { y[0] = p[g]; y[1] = p[g + 1]; y[2] = p[g + 2]; y[3] = p[g + 3]; }
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = __fmul_rn(__fmul_rn(v[q], __fsub_rn(1.0f, y[q])), y[q]);
        }
        int r = g / cw, c = g - r * cw;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            tile[(size_t)(r0 + r) * ld + c] = v[q];
            if (++c == cw) { c = 0; ++r; }
        }
    }
    for (int g = head + 4 * nb + tid; g < n; g += nth) one(g);
}

__device__ inline void tile_load(const float *in_row0, const float *p_row0, int row, int c0, int cw, int cnt, float *tile, int ld) {
    if (cw == row) {
        span_load(in_row0, p_row0, cnt * cw, tile, ld, cw, 0, (int)threadIdx.x, kThreads);
    } else {
        for (int r = (int)(threadIdx.x >> 6); r < cnt; r += kWaves)
            span_load(in_row0 + (size_t)r * row + c0, p_row0 ? p_row0 + (size_t)r * row + c0 : nullptr, cw, tile, ld, cw, r,
                      (int)(threadIdx.x & 63), kWave);
    }
}

// the tile's columns [0, cw) -> planes [ch0, ch0 + cw) of a level's gradient map: a wave per plane, a lane per anchor
template <int kDt>
__device__ inline void tile_to_planes(void *__restrict__ map, int b, int chans, int n, int a0, int cnt, int ch0, int cw,
                                      const float *tile, int ld) {
    typedef typename DetheadMap<kDt>::elem E;
    const int lane = (int)(threadIdx.x & 63);
    if (lane >= cnt) return;
    for (int c = (int)(threadIdx.x >> 6); c < cw; c += kWaves)
        dethead_store<kDt>(static_cast<E *>(map) + ((size_t)b * chans + (size_t)(ch0 + c)) * (size_t)n + (size_t)(a0 + lane),
                           tile[(size_t)lane * ld + c]);
}

template <int kDt>
__global__ __launch_bounds__(kThreads) void k_dethead_backward(const DetheadArgs t) {
    __shared__ float tile[kDetheadLds];
    int l, a0, cnt;
    dethead_tile(t, l, a0, cnt);
    const int b = blockIdx.y, n = t.n[l];
    const size_t at = (size_t)b * t.N + (size_t)(t.off[l] + a0);
    if (t.gs) {
        for (int c0 = 0; c0 < t.nc; c0 += kDetheadCols) {
            const int cw = t.nc - c0 < kDetheadCols ? t.nc - c0 : kDetheadCols, ld = cw | 1;
            tile_load(t.gs + at * (size_t)t.nc, t.p + at * (size_t)t.nc, t.nc, c0, cw, cnt, tile, ld);
            __syncthreads();
            tile_to_planes<kDt>(t.gcls[l], b, t.nc, n, a0, cnt, c0, cw, tile, ld);
            __syncthreads();
        }
    }
    if (t.gd) {
        const int row = 4 * t.K, ld = row | 1;
        tile_load(t.gd + at * (size_t)row, nullptr, row, 0, row, cnt, tile, ld);
        __syncthreads();
        tile_to_planes<kDt>(t.greg[l], b, row, n, a0, cnt, 0, row, tile, ld);
    }
}

}  // namespace evrep
