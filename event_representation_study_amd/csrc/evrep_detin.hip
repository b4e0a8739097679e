// evrep_detin.hip -- the detector's input batch in one launch (r07): a channel-last (B, H, W, C) representation -> the
// channel-first (B, C, S, S) float32 tensor the detector eats.  What Gen1H5.__getitem__ does after get_item_transform, plus
// collate_fn and Trainer.prepro_data (ev-YOLOv6/yolov6/data/gen1_2yolo.py:230-265,320-398,427-447; data_augment.py:31-85,
// 110-184; yolov6/core/engine.py:629-635): keep-ratio resize, letterbox, random_affine's warp, the two flips, HWC -> CHW with
// [::-1], .float() / 255.  Every output element evaluates the composition below; none of the intermediate images exists in
// memory.  T is the input's dtype; no multiply is fused with an add (-ffp-contract=off).
//
//   R  resize     R(b, y, x, c) = what k_resize_taps writes with scale 1 and output dtype T: over the y taps, in tap order, of
//                 (over the x taps, in tap order, of src * xwt) * ywt, both sums in float64, then one cast to T.  The per-axis
//                 tables come from the host (gwd_pipeline.resize_taps: OpenCV's published INTER_AREA / INTER_LINEAR tables);
//                 one tap of weight 1 per row and column reproduces the source bit for bit.
//   L  letterbox  I(b, y, x, c) = R(b, y - top, x - left, c) inside the nh x nw rectangle, pad[c] elsewhere in the S x S square.
//   W  warp       only for a sample whose flag has EVREP_DETIN_WARP: cv2.warpAffine(I, M[:2], dsize=(S, S), borderValue=pad) with
//                 its defaults (INTER_LINEAR, BORDER_CONSTANT), RESTATED from OpenCV's published algorithm (imgwarp.cpp:
//                 warpAffine -> WarpAffineInvoker -> remap's bilinear pass for floating-point images) -- PARITY UNPINNED
//                 against cv2 itself, which is absent.  OpenCV inverts M in float64 (D = M00 M11 - M01 M10; D = D != 0 ? 1/D :
//                 0; m00 = M11 D, m11 = M00 D, m01 = -M01 D, m10 = -M10 D, m02 = -m00 M02 - m01 M12, m12 = -m10 M02 - m11 M12)
//                 and walks the inverse map in 10-bit fixed point (AB_BITS = 10, rounding half to even):
//                     adelta[x] = rint(m00 x 1024),  bdelta[x] = rint(m10 x 1024)
//                     X0[y] = rint((m01 y + m02) 1024) + 16,  Y0[y] = rint((m11 y + m12) 1024) + 16
//                     X = (X0[y] + adelta[x]) >> 5,  Y = (Y0[y] + bdelta[x]) >> 5          (arithmetic shifts: 5 fractional bits left)
//                     sx = clamp(X >> 5, -32768, 32767), sy likewise (the map is stored as int16), ax = (X & 31) / 32, ay = (Y & 31) / 32
//                 and the value, in dtype T, is ((v00 w00 + v01 w01) + v10 w10) + v11 w11 with w00 = (1-ay)(1-ax), w01 = (1-ay) ax,
//                 w10 = ay (1-ax), w11 = ay ax (all exact in float32), v00 at (sy, sx), v01 at (sy, sx+1), v10 at (sy+1, sx),
//                 v11 at (sy+1, sx+1); a tap outside [0, S) takes pad[c].  The four integer tables of a sample are made on the
//                 host in int64 (detector_input.warp_tables), which refuses entries or sums outside int32 -- where OpenCV's own
//                 int arithmetic would overflow; the kernel adds them in 64 bits all the same.
//   F  flips      F(b, y, x, c) = W(b, S-1-y if EVREP_DETIN_FLIPUD, S-1-x if EVREP_DETIN_FLIPLR, c)
//      convert    out[b, c, y, x] = fl32(F(b, y, x, C-1-c)) * scale   (scale = fl32(1/255): torch's `.float() / 255`)
//
// A workgroup owns P = 256 / G consecutive output pixels of one sample (row-major over the S x S plane), G = ceil(C / 4); a thread
// computes one pixel's group of four channels, group fastest over the lanes.  The C values of a source pixel are contiguous
// (channel last), so neighbouring lanes load neighbouring 4-channel pieces of the same source pixel, then of the next one:
// a wave's load touches a third of the cache lines it would with a pixel per lane, 96 or 192 bytes between lanes (measured,
// 32 x 12 x 640 x 640 in train mode: from 1280x720 4.2 -> 2.2 ms, from 304x240 1.7 -> 1.6 ms).  The results meet in a [C][P] float tile in LDS and leave
// from there channel plane by channel plane: every store of a wave is a run of consecutive floats of one plane.  The
// source (a few MB per window) is read through the caches: every output pixel touches at most 4 (warp) x Ty x Tx source
// pixels, shared with its neighbours.  Every index is brought into range before any load: a letterbox coordinate outside
// the rectangle takes the pad, tap rows and columns are clamped to the source, tap counts to T, and the warp's taps are
// compared with [0, S) after the int16 clamp.
// grid (ceil(S*S / P), B), 256 threads, 16 KB of LDS.
#pragma once
#include "evrep_common.h"

namespace evrep {

constexpr int kDetinGroup = 4;   // channels per pass of a thread

template <typename T>
struct DetinArgs {
    const T *src;                                       // (B, H, W, C)
    const int32_t *ystart, *ycount, *xstart, *xcount;  // [nh], [nh], [nw], [nw]
    const double *ywt, *xwt;                            // [nh][Tt], [nw][Tt]
    const double *pad;                                  // [C]
    const uint32_t *flags;                              // [B] or NULL (no sample warps or flips)
    const int32_t *warp;                                // [B][4][S]: adelta, bdelta, X0, Y0; read only where the flag asks
    float *out;                                         // (B, C, S, S)
    int32_t H, W, C, nh, nw, Tt, S, top, left;
    float scale;
};

// I(b, iy, ix, c0 + j) for j < n (n <= kDetinGroup) into v
template <typename T>
__device__ __forceinline__ void detin_letterboxed(const DetinArgs<T> &a, const T *__restrict__ src, int iy, int ix, int c0, int n,
                                                  const T (&padv)[kDetinGroup], T (&v)[kDetinGroup]) {
    const int ry = iy - a.top, rx = ix - a.left;
    if (iy < 0 || iy >= a.S || ix < 0 || ix >= a.S || ry < 0 || ry >= a.nh || rx < 0 || rx >= a.nw) {
#pragma unroll
        for (int j = 0; j < kDetinGroup; ++j) v[j] = padv[j];
        return;
    }
    const int ys = a.ystart[ry], xs = a.xstart[rx];
    const int yn = min(max(a.ycount[ry], 0), a.Tt), xn = min(max(a.xcount[rx], 0), a.Tt);
    const double *__restrict__ yw = a.ywt + (size_t)ry * a.Tt, *__restrict__ xw = a.xwt + (size_t)rx * a.Tt;
    double acc[kDetinGroup];
#pragma unroll
    for (int j = 0; j < kDetinGroup; ++j) acc[j] = 0.0;
    for (int ty = 0; ty < yn; ++ty) {
        const int sy = min(max(ys + ty, 0), a.H - 1);
        const T *__restrict__ row = src + (size_t)sy * a.W * a.C + c0;
        double rsum[kDetinGroup];
#pragma unroll
        for (int j = 0; j < kDetinGroup; ++j) rsum[j] = 0.0;
        for (int tx = 0; tx < xn; ++tx) {
            const int sx = min(max(xs + tx, 0), a.W - 1);
            const double w = xw[tx];
            const T *__restrict__ px = row + (size_t)sx * a.C;
#pragma unroll
            for (int j = 0; j < kDetinGroup; ++j)
                if (j < n) rsum[j] += (double)px[j] * w;
        }
        const double wy = yw[ty];
#pragma unroll
        for (int j = 0; j < kDetinGroup; ++j) acc[j] += rsum[j] * wy;
    }
#pragma unroll
    for (int j = 0; j < kDetinGroup; ++j) v[j] = (T)acc[j];
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_detector_input(const DetinArgs<T> a) {
    __shared__ float tile[EVREP_MAX_CHANNELS * kThreads];   // [C][P] of this block's results, P <= kThreads
    const int S = a.S, C = a.C;
    const int G = (C + kDetinGroup - 1) / kDetinGroup, P = kThreads / G;   // channel groups; pixels of a block
    const int b = blockIdx.y;
    const int p0 = blockIdx.x * P;                         // S <= 4096: S * S fits
    const int npx = min(P, S * S - p0);
    const int lp = threadIdx.x / G, grp = threadIdx.x - lp * G;
    if (lp < npx) {
        const int e = p0 + lp;
        const int oy = e / S, ox = e - oy * S;
        const uint32_t flag = a.flags ? a.flags[b] : 0u;
        const int y = (flag & EVREP_DETIN_FLIPUD) ? S - 1 - oy : oy;
        const int x = (flag & EVREP_DETIN_FLIPLR) ? S - 1 - ox : ox;
        const bool warp = (flag & EVREP_DETIN_WARP) != 0u && a.warp != nullptr;
        int sx = x, sy = y;
        T w00 = (T)1, w01 = (T)0, w10 = (T)0, w11 = (T)0;
        if (warp) {
            const int32_t *__restrict__ tab = a.warp + (size_t)b * 4 * S;
            const int64_t X = ((int64_t)tab[2 * S + y] + (int64_t)tab[x]) >> 5;
            const int64_t Y = ((int64_t)tab[3 * S + y] + (int64_t)tab[S + x]) >> 5;
            const int64_t cx = X >> 5, cy = Y >> 5;
            sx = (int)(cx < -32768 ? -32768 : (cx > 32767 ? 32767 : cx));
            sy = (int)(cy < -32768 ? -32768 : (cy > 32767 ? 32767 : cy));
            const T ax = (T)(int)(X & 31) / (T)32, ay = (T)(int)(Y & 31) / (T)32;
            w00 = ((T)1 - ay) * ((T)1 - ax);
            w01 = ((T)1 - ay) * ax;
            w10 = ay * ((T)1 - ax);
            w11 = ay * ax;
        }
        const T *__restrict__ src = a.src + (size_t)b * a.H * a.W * C;
        const int c0 = grp * kDetinGroup;
        const int n = min(kDetinGroup, C - c0);
        T padv[kDetinGroup], v[kDetinGroup];
#pragma unroll
        for (int j = 0; j < kDetinGroup; ++j) padv[j] = (T)a.pad[min(c0 + j, C - 1)];
        detin_letterboxed(a, src, sy, sx, c0, n, padv, v);
        if (warp) {
            T v01[kDetinGroup], v10[kDetinGroup], v11[kDetinGroup];
            detin_letterboxed(a, src, sy, sx + 1, c0, n, padv, v01);
            detin_letterboxed(a, src, sy + 1, sx, c0, n, padv, v10);
            detin_letterboxed(a, src, sy + 1, sx + 1, c0, n, padv, v11);
#pragma unroll
            for (int j = 0; j < kDetinGroup; ++j) v[j] = ((v[j] * w00 + v01[j] * w01) + v10[j] * w10) + v11[j] * w11;
        }
#pragma unroll
        for (int j = 0; j < kDetinGroup; ++j)
            if (j < n) tile[(C - 1 - (c0 + j)) * P + lp] = (float)v[j] * a.scale;
    }
    __syncthreads();
    float *__restrict__ out = a.out + (size_t)b * C * S * S + p0;
    for (int i = threadIdx.x; i < C * npx; i += kThreads) {
        const int c = i / npx, px = i - c * npx;
        out[(size_t)c * S * S + px] = tile[c * P + px];
    }
}

}  // namespace evrep
