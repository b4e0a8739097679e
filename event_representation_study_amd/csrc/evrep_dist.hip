// evrep_dist.hip -- N-ImageNet's DiST image (n_imagenet/real_cnn_model/data/imagenet.py:873-999, reshape_then_acc_adj_sort) for
// the B windows of a batch, from the (B, H, W, 6) float32 output of k_polstats [pos count, pos latest, pos earliest, neg count,
// neg latest, neg earliest], and the dense rank it ends in as a primitive of its own.  Every (window, polarity) image is one
// SEGMENT.  Three stages, each the reference's statements in plain IEEE float32 operations (the library is built with
// -ffp-contract=off; every division is __fdiv_rn):
//
//   k_dist_clip     one workgroup per segment.  th = #{ j : S_j < H*W*clip_rate }, S_j the running pixel count over the DISTINCT
//                   count values in ascending order (:897-906); both sides in float32, as torch compares an int64 tensor with a
//                   Python float (S_j <= 2^24 is exact there, the float64 product is rounded once).  An LDS histogram over a window of kClipBins count values
//                   [base, base + kClipBins); while the running count has not reached the limit the window moves on to the
//                   smallest count beyond it (found in the same sweep), so the result is exact for any counts, however sparse.
//   k_dist_stencil  one workgroup per 16 x 64 tile and segment.  Clipped count, latest time and -earliest time (earliest = 1
//                   where the clipped count is 0) of the tile and its two-pixel halo go to LDS once; the 5x5 sum (zero padding)
//                   and the two 5x5 maxima (-inf padding) are taken separably (sums of small integers and maxima do not depend
//                   on the order); nb = 25 * (s / 25); disc = (max + max) / nb; out -= alpha * disc where count > 0; out < 0 -> 0;
//                   nb == 1 -> 0 (:926-968).  One float per pixel leaves the kernel.
//   k_dense_rank    one workgroup per segment.  out[i] = #{distinct keys < key[i]} / #{distinct keys} (:970-990).  A stable LSD
//                   radix sort of (key, index) pairs through global scratch, four passes of eight bits: per pass a digit
//                   histogram (wave_match: one LDS atomic per wave and distinct digit), then chunks of 4 096 pairs in order --
//                   every wave ranks its 256 pairs against its own row of per-digit counters, the rows are scanned over the
//                   sixteen waves on top of the running digit bases, and the pairs are scattered.  Then head flags, a count of
//                   them (the divisor) and a chunked scan that writes rank / n at each pair's index.  Keys are ordered as floats
//                   (negative ones too); -0.0 counts as +0.0.
// Nothing here waits for the device or reads a size on the host.
#pragma once
#include "evrep_common.h"
#include "evrep_ranksort.h"                           // kDistThreads, rank_key, rank_pair_sort: shared with evrep_sort.hip

namespace evrep {

constexpr int kClipBins = 4096;                       // count values one sweep of the clip resolves (four bins per thread)
constexpr int kTileH = 16, kTileW = 64, kHalo = 2;    // the stencil's tile; 256 threads, four pixels each
constexpr int kStencilThreads = 256;
static_assert(kClipBins == 4 * kDistThreads, "k_dist_clip gives every thread four bins");

// ------------------------------------------------------------------------------------------------------------- stage (a)
__global__ __launch_bounds__(kDistThreads) void k_dist_clip(const float *__restrict__ prim, int npx, float limit, uint32_t *__restrict__ th_out) {
    __shared__ uint32_t hist[kClipBins];
    __shared__ uint32_t scan_tmp[kDistWaves];
    __shared__ uint32_t s_next;
    const int tid = threadIdx.x, lane = tid & 63;
    const int seg = blockIdx.x;
    const float *cnt = prim + (size_t)(seg >> 1) * (size_t)npx * 6u + (size_t)(seg & 1) * 3u;
    uint32_t base = 0, th = 0;
    uint64_t cum = 0;                                    // pixels with a count below `base` (the same in every thread)
    for (;;) {
#pragma unroll
        for (int q = 0; q < 4; ++q) hist[tid + q * kDistThreads] = 0;
        if (tid == 0) s_next = 0xFFFFFFFFu;
        __syncthreads();
        for (int i0 = 0; i0 < npx; i0 += kDistThreads) {
            const int i = i0 + tid;
            const uint32_t c = i < npx ? (uint32_t)cnt[(size_t)i * 6u] : 0u;
            const bool in_win = i < npx && c >= base && c - base < (uint32_t)kClipBins;
            if (i < npx && c >= base && !in_win) atomicMin(&s_next, c);
            // equal counts are the rule (most pixels hold 0, 1 or 2 events): one atomic per wave and distinct value
            uint64_t todo = __ballot(in_win);
            while (todo) {
                const int leader = __ffsll((unsigned long long)todo) - 1;
                const uint32_t lc = (uint32_t)__shfl((int)c, leader, 64);
                const uint64_t same = __ballot(in_win && c == lc);
                if (lane == leader) atomicAdd(&hist[lc - base], (uint32_t)__popcll(same));
                todo &= ~same;
            }
        }
        __syncthreads();
        uint32_t h[4], sum = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { h[q] = hist[tid * 4 + q]; sum += h[q]; }
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<kDistWaves>(sum, scan_tmp, &tot);
        uint64_t run = cum + ex;
        uint32_t good = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (h[q]) { run += h[q]; good += ((float)run < limit) ? 1u : 0u; }      // S_j < H*W*clip_rate, in float32 as torch compares
        }
        uint32_t good_tot;
        block_exclusive_scan<kDistWaves>(good, scan_tmp, &good_tot);
        th += good_tot;
        cum += tot;
        const uint32_t next = s_next;
        if (!((float)cum < limit) || next == 0xFFFFFFFFu) break;      // every later S_j is >= limit / no count is left
        base = next;
        __syncthreads();                                             // s_next and hist are rewritten
    }
    if (tid == 0) th_out[seg] = th;
}

// ------------------------------------------------------------------------------------------------------------- stage (b)
__global__ __launch_bounds__(kStencilThreads) void k_dist_stencil(const float *__restrict__ prim, int H, int W, int tiles_x, int tiles,
                                                                  const uint32_t *__restrict__ th_in, float alpha, float *__restrict__ keys) {
    constexpr int IH = kTileH + 2 * kHalo, IW = kTileW + 2 * kHalo;
    __shared__ float in[3][IH][IW];          // clipped count, latest, -earliest
    __shared__ float row[3][IH][kTileW];     // the same, over five columns
    const int tid = threadIdx.x;
    const int seg = blockIdx.x / tiles, tile = blockIdx.x - seg * tiles;
    const int ty0 = (tile / tiles_x) * kTileH, tx0 = (tile % tiles_x) * kTileW;
    const size_t npx = (size_t)H * (size_t)W;
    const float *src = prim + (size_t)(seg >> 1) * npx * 6u + (size_t)(seg & 1) * 3u;
    const float th = (float)th_in[seg];
    const float ninf = -__builtin_inff();
    for (int idx = tid; idx < IH * IW; idx += kStencilThreads) {
        const int ry = idx / IW, rx = idx - ry * IW;
        const int y = ty0 + ry - kHalo, x = tx0 + rx - kHalo;
        float c = 0.0f, o = ninf, nm = ninf;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const float *p = src + ((size_t)y * (size_t)W + (size_t)x) * 6u;
            c = fminf(p[0], th);                           // count[count > th] = th
            o = p[1];
            nm = -(c == 0.0f ? 1.0f : p[2]);               // min_out[count == 0] = 1
        }
        in[0][ry][rx] = c;
        in[1][ry][rx] = o;
        in[2][ry][rx] = nm;
    }
    __syncthreads();
    for (int idx = tid; idx < IH * kTileW; idx += kStencilThreads) {
        const int ry = idx / kTileW, cx = idx - ry * kTileW;
        float s = in[0][ry][cx], m1 = in[1][ry][cx], m2 = in[2][ry][cx];
#pragma unroll
        for (int d = 1; d < 5; ++d) {
            s += in[0][ry][cx + d];
            m1 = fmaxf(m1, in[1][ry][cx + d]);
            m2 = fmaxf(m2, in[2][ry][cx + d]);
        }
        row[0][ry][cx] = s;
        row[1][ry][cx] = m1;
        row[2][ry][cx] = m2;
    }
    __syncthreads();
    float *dst = keys + (size_t)seg * npx;
#pragma unroll
    for (int q = 0; q < kTileH * kTileW / kStencilThreads; ++q) {
        const int idx = tid + q * kStencilThreads;
        const int py = idx / kTileW, px = idx - py * kTileW;
        const int y = ty0 + py, x = tx0 + px;
        if (y >= H || x >= W) continue;
        float s = row[0][py][px], m1 = row[1][py][px], m2 = row[2][py][px];
#pragma unroll
        for (int d = 1; d < 5; ++d) {
            s += row[0][py + d][px];
            m1 = fmaxf(m1, row[1][py + d][px]);
            m2 = fmaxf(m2, row[2][py + d][px]);
        }
        const float c = in[0][py + kHalo][px + kHalo];
        float o = in[1][py + kHalo][px + kHalo];
        const float nb = 25.0f * __fdiv_rn(s, 25.0f);      // patch_size**2 * avg_pool2d(count): the reference's two statements
        const float disc = __fdiv_rn(m1 + m2, nb);
        if (c > 0.0f) {
            const float ad = alpha * disc;                 // a multiply and a subtract of their own (no FMA)
            o = o - ad;
        }
        if (o < 0.0f) o = 0.0f;
        if (nb == 1.0f) o = 0.0f;
        gstore_f32(dst + (size_t)y * (size_t)W + (size_t)x, o);
    }
}

// ------------------------------------------------------------------------------------------------------------- stage (c)
struct RankArgs {
    const float *keys;          // segment s = keys [o0, o0 + n)
    const int64_t *offsets;     // S + 1 entries, or nullptr: every segment holds `uniform_len` keys
    int64_t uniform_len;
    int32_t S;
    char *scratch;              // four uint32 arrays of rank_array_bytes(total) each, indexed like `keys`: keys a, indices a, keys b, indices b
    float *out;
    int32_t *n_distinct;        // S entries or nullptr
};
// total = offsets[S] (read on the device) or S * uniform_len; every array holds rank_array_bytes(total) bytes

__global__ __launch_bounds__(kDistThreads) void k_dense_rank(const RankArgs a) {
    __shared__ RankSortLds lds;
    uint32_t *const scan_tmp = lds.scan_tmp;
    const int tid = threadIdx.x;
    const int seg = blockIdx.x;
    int64_t o0, n, total;
    if (a.offsets) {
        o0 = a.offsets[seg];
        n = a.offsets[seg + 1] - o0;
        total = a.offsets[a.S];
    } else {
        o0 = (int64_t)seg * a.uniform_len;
        n = a.uniform_len;
        total = (int64_t)a.S * a.uniform_len;
    }
    if (o0 + n > total) n = 0;                            // (offsets that do not ascend: the segment is left alone)
    if (n <= 0 || o0 < 0) {
        if (a.n_distinct && tid == 0) a.n_distinct[seg] = 0;
        return;
    }
    const float *keys = a.keys + o0;
    const size_t ab = rank_array_bytes(total);
    uint32_t *const ka = reinterpret_cast<uint32_t *>(a.scratch) + o0, *const ia = reinterpret_cast<uint32_t *>(a.scratch + ab) + o0;
    uint32_t *const kb = reinterpret_cast<uint32_t *>(a.scratch + 2 * ab) + o0, *const ib = reinterpret_cast<uint32_t *>(a.scratch + 3 * ab) + o0;

    rank_pair_sort([keys](int64_t i) { return rank_key(keys[i]); }, n, ka, ia, kb, ib, lds);

    // sorted pairs are in the second buffers.  Heads, their number, then rank / number at every pair's index.
    const uint32_t *ks = kb, *is = ib;
    uint32_t heads = 0;
    for (int64_t i = tid; i < n; i += kDistThreads) heads += (i == 0 || ks[i] != ks[i - 1]) ? 1u : 0u;
    uint32_t ndist;
    block_exclusive_scan<kDistWaves>(heads, scan_tmp, &ndist);
    if (a.n_distinct && tid == 0) a.n_distinct[seg] = (int32_t)ndist;
    const float fn = (float)ndist;
    float *out = a.out + o0;
    uint32_t running = 0;                                 // heads in front of this round
    for (int64_t i0 = 0; i0 < n; i0 += kDistThreads) {
        const int64_t i = i0 + tid;
        const uint32_t h = (i < n && (i == 0 || ks[i] != ks[i - 1])) ? 1u : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<kDistWaves>(h, scan_tmp, &tot);
        if (i < n) gstore_f32(out + is[i], __fdiv_rn((float)(running + ex + h - 1u), fn));
        running += tot;
    }
}

}  // namespace evrep
