// evrep_detin_frames.hip -- the detector's input batch for frames of DIFFERENT sizes (TORE's bounding boxes) in one launch, and
// the resize tap tables made on the device.  Beside evrep_detin.hip: the same output mapping, the same [C][P] LDS tile, the same
// composition F o W o L per output element (see there for W, F and the conversion); only the letterboxed read changes.  A
// workgroup reads its sample's evrep_detin_frame (uniform over the workgroup):
//
//   R1 stage 1   R1(y, x, c) = what k_resize_taps writes for this frame alone: over the y taps of (over the x taps of
//                src * xw1) * yw1, both sums in float64 in tap order, one cast to T.  rh x rw values.
//   R  stage 2   T2 == 0 (letterbox needs no resize of its own, nh x nw == rh x rw):  R = R1.
//                T2 > 0:  R(y, x, c) = (T) sum_ty (sum_tx (double)R1(ys2 + ty, xs2 + tx, c) * xw2) * yw2 -- what
//                resize_batch(resize_batch(frame, rh, rw, interp), nh, nw, "linear") computes through an rh x rw image in
//                memory; here every R1 value is evaluated where it is needed, up to 2 x 2 of them per letterboxed tap.
//   L            I(y, x, c) = R(y - top, x - left, c) inside the nh x nw rectangle, pad[c] elsewhere in the S x S square.
//
// All tap tables of a batch lie in three arrays (start[n_rows], count[n_rows], weights[n_wt]); an axis is a run of rows
// at a row offset with T weights per row at a weight offset.  k_resize_tap_tables fills them, one lane per output index of
// an axis, with the arithmetic of gwd_pipeline.area_weights / linear_weights statement for statement in float64 (IEEE basic
// operations only; -ffp-contract=off), trimmed to the non-zero run as gwd_pipeline.resize_taps trims it.
//
// Every index taken from a device table is brought into range before a load: table rows to [0, n_rows), weight runs to
// [0, n_wt), counts to T, tap rows / columns to the frame (stage 1) or the rh x rw rectangle (stage 2), the warp's taps are
// compared with [0, S).  No multiply is fused with an add.
// k_detector_input_frames: grid (ceil(S*S / P), B), 256 threads, 16 KB of LDS.  k_resize_tap_tables: grid (n_axes,
// ceil(max dst / 256)), 256 threads.
#pragma once
#include "evrep_detin.hip"

namespace evrep {

// ------------------------------------------------------------------------------------------------ tap tables
struct TapTableArgs {
    const int32_t *axes;      // [n_axes][6]: src, dst, interpolation, T, row offset, weight offset
    int32_t *start, *count;   // [n_rows]
    double *wt;               // [n_wt]
    int64_t n_rows, n_wt;
    int32_t n_axes;
};

__global__ __launch_bounds__(kThreads) void k_resize_tap_tables(const TapTableArgs a) {
    const int32_t *__restrict__ ax = a.axes + (size_t)blockIdx.x * 6;
    const int src = ax[0], dst = ax[1], interp = ax[2], T = ax[3];
    const int d = blockIdx.y * kThreads + threadIdx.x;
    if (src < 1 || dst < 1 || T < 1 || d >= dst) return;
    const int64_t row = (int64_t)ax[4] + d, w0 = (int64_t)ax[5] + (int64_t)d * T;
    if (ax[4] < 0 || ax[5] < 0 || row >= a.n_rows || w0 + T > a.n_wt) return;   // a run that leaves the tables is not written
    int first = 0, n = 0;
    double we0 = 0.0, wmid = 0.0, wlast = 0.0;   // the run: [we0 if it starts before s1] wmid ... wmid [wlast]
    bool lead = false, tail = false;
    if (interp == EVREP_TAPS_AREA) {
        const double scale = (double)src / (double)dst;
        const double f1 = (double)d * scale;
        const double f2 = f1 + scale;
        const double rest = (double)src - f1;
        const double cell = scale < rest ? scale : rest;
        int s1 = (int)ceil(f1);
        const int fl = (int)floor(f2);
        const int s2 = fl < src - 1 ? fl : src - 1;
        s1 = s1 < s2 ? s1 : s2;
        lead = (double)s1 - f1 > 1e-3;
        tail = f2 - (double)s2 > 1e-3;
        if (lead) we0 = ((double)s1 - f1) / cell;
        wmid = 1.0 / cell;
        if (tail) {
            double m = f2 - (double)s2;
            m = 1.0 < m ? 1.0 : m;
            m = cell < m ? cell : m;
            wlast = m / cell;
        }
        first = lead ? s1 - 1 : s1;
        n = (lead ? 1 : 0) + (s2 - s1) + (tail ? 1 : 0);
    } else if (interp == EVREP_TAPS_LINEAR) {
        const double scale = (double)src / (double)dst;
        double fx = ((double)d + 0.5) * scale - 0.5;
        const double fl = floor(fx);
        int sx = (int)fl;
        fx -= fl;
        if (sx < 0) { sx = 0; fx = 0.0; }
        if (sx >= src - 1) { sx = src - 1; fx = 0.0; }
        // the row holds 1 - fx at sx and, where fx != 0, fx at sx + 1; zero entries at either end are trimmed
        const double a0 = 1.0 - fx;
        if (a0 != 0.0) { first = sx; lead = true; we0 = a0; tail = fx != 0.0; wlast = fx; }
        else if (fx != 0.0) { first = sx + 1; tail = true; wlast = fx; }
        n = (lead ? 1 : 0) + (tail ? 1 : 0);
    } else if (interp == EVREP_TAPS_IDENTITY) {   // one tap of weight 1
        first = d < src ? d : src - 1;
        lead = true;
        we0 = 1.0;
        n = 1;
    } else {
        return;
    }
    if (n <= 0) { first = 0; n = 0; }
    const int nw = n < T ? n : T;
    a.start[row] = first;
    a.count[row] = n;
    for (int t = 0; t < T; ++t) {
        double w = 0.0;
        if (t < nw) w = (lead && t == 0) ? we0 : ((tail && t == n - 1) ? wlast : wmid);
        a.wt[w0 + t] = w;
    }
}

// ------------------------------------------------------------------------------------------------ the frames launch
template <typename T>
struct DetinFramesArgs {
    const evrep_detin_frame *frames;       // [B], the validated copy on the device
    const int32_t *tstart, *tcount;        // [n_rows]
    const double *twt;                     // [n_wt]
    const double *pad;                     // [C]
    const int32_t *warp;                   // [B][4][S] or NULL
    float *out;                            // (B, C, S, S)
    int64_t n_rows, n_wt;
    int32_t C, S;
    float scale;
};

// one axis entry: the first tap, the number of taps (<= Tc) and where its weights start, all in range
struct DetinTap {
    int start, n;
    const double *w;
};

template <typename T>
__device__ __forceinline__ DetinTap detin_tap(const DetinFramesArgs<T> &a, int32_t row_off, int32_t wt_off, int i, int Tt) {
    const int64_t r = min(max((int64_t)row_off + i, (int64_t)0), a.n_rows - 1);
    const int Tc = (int)min((int64_t)max(Tt, 0), a.n_wt);
    const int64_t w = min(max((int64_t)wt_off + (int64_t)i * Tt, (int64_t)0), a.n_wt - Tc);
    DetinTap t;
    t.start = a.tstart[r];
    t.n = min(max(a.tcount[r], 0), Tc);
    t.w = a.twt + w;
    return t;
}

// R1(ry, rx, c0 + j) for j < n into v; ry, rx are brought into the rh x rw rectangle
template <typename T>
__device__ __forceinline__ void detin_stage1(const DetinFramesArgs<T> &a, const evrep_detin_frame &f, const T *__restrict__ src, int ry,
                                             int rx, int c0, int n, T (&v)[kDetinGroup]) {
    ry = min(max(ry, 0), f.rh - 1);
    rx = min(max(rx, 0), f.rw - 1);
    const DetinTap ty = detin_tap(a, f.row1, f.wrow1, ry, f.T1), tx = detin_tap(a, f.col1, f.wcol1, rx, f.T1);
    double acc[kDetinGroup];
#pragma unroll
    for (int j = 0; j < kDetinGroup; ++j) acc[j] = 0.0;
    for (int iy = 0; iy < ty.n; ++iy) {
        const int sy = min(max(ty.start + iy, 0), f.H - 1);
        const T *__restrict__ row = src + (size_t)sy * f.W * a.C + c0;
        double rsum[kDetinGroup];
#pragma unroll
        for (int j = 0; j < kDetinGroup; ++j) rsum[j] = 0.0;
        for (int ix = 0; ix < tx.n; ++ix) {
            const int sx = min(max(tx.start + ix, 0), f.W - 1);
            const double w = tx.w[ix];
            const T *__restrict__ px = row + (size_t)sx * a.C;
#pragma unroll
            for (int j = 0; j < kDetinGroup; ++j)
                if (j < n) rsum[j] += (double)px[j] * w;
        }
        const double wy = ty.w[iy];
#pragma unroll
        for (int j = 0; j < kDetinGroup; ++j) acc[j] += rsum[j] * wy;
    }
#pragma unroll
    for (int j = 0; j < kDetinGroup; ++j) v[j] = (T)acc[j];
}

// I(iy, ix, c0 + j) for j < n into v
template <typename T>
__device__ __forceinline__ void detin_frame_letterboxed(const DetinFramesArgs<T> &a, const evrep_detin_frame &f, const T *__restrict__ src,
                                                        int iy, int ix, int c0, int n, const T (&padv)[kDetinGroup],
                                                        T (&v)[kDetinGroup]) {
    const int ry = iy - f.top, rx = ix - f.left;
    if (iy < 0 || iy >= a.S || ix < 0 || ix >= a.S || ry < 0 || ry >= f.nh || rx < 0 || rx >= f.nw) {
#pragma unroll
        for (int j = 0; j < kDetinGroup; ++j) v[j] = padv[j];
        return;
    }
    if (f.T2 <= 0) {
        detin_stage1(a, f, src, ry, rx, c0, n, v);
        return;
    }
    const DetinTap ty = detin_tap(a, f.row2, f.wrow2, ry, f.T2), tx = detin_tap(a, f.col2, f.wcol2, rx, f.T2);
    double acc[kDetinGroup];
#pragma unroll
    for (int j = 0; j < kDetinGroup; ++j) acc[j] = 0.0;
    for (int jy = 0; jy < ty.n; ++jy) {
        double rsum[kDetinGroup];
#pragma unroll
        for (int j = 0; j < kDetinGroup; ++j) rsum[j] = 0.0;
        for (int jx = 0; jx < tx.n; ++jx) {
            T r1[kDetinGroup];
            detin_stage1(a, f, src, ty.start + jy, tx.start + jx, c0, n, r1);
            const double w = tx.w[jx];
#pragma unroll
            for (int j = 0; j < kDetinGroup; ++j) rsum[j] += (double)r1[j] * w;
        }
        const double wy = ty.w[jy];
#pragma unroll
        for (int j = 0; j < kDetinGroup; ++j) acc[j] += rsum[j] * wy;
    }
#pragma unroll
    for (int j = 0; j < kDetinGroup; ++j) v[j] = (T)acc[j];
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_detector_input_frames(const DetinFramesArgs<T> a) {
    __shared__ float tile[EVREP_MAX_CHANNELS * kThreads];   // [C][P] of this block's results, P <= kThreads
    const int S = a.S, C = a.C;
    const int G = (C + kDetinGroup - 1) / kDetinGroup, P = kThreads / G;   // channel groups; pixels of a block
    const int b = blockIdx.y;
    const int p0 = blockIdx.x * P;                         // S <= 4096: S * S fits
    const int npx = min(P, S * S - p0);
    const int lp = threadIdx.x / G, grp = threadIdx.x - lp * G;
    if (lp < npx) {
        const evrep_detin_frame f = a.frames[b];
        const int e = p0 + lp;
        const int oy = e / S, ox = e - oy * S;
        const uint32_t flag = f.flags;
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
        const T *__restrict__ src = static_cast<const T *>(f.src);
        const int c0 = grp * kDetinGroup;
        const int n = min(kDetinGroup, C - c0);
        T padv[kDetinGroup], v[kDetinGroup];
#pragma unroll
        for (int j = 0; j < kDetinGroup; ++j) padv[j] = (T)a.pad[min(c0 + j, C - 1)];
        detin_frame_letterboxed(a, f, src, sy, sx, c0, n, padv, v);
        if (warp) {
            T v01[kDetinGroup], v10[kDetinGroup], v11[kDetinGroup];
            detin_frame_letterboxed(a, f, src, sy, sx + 1, c0, n, padv, v01);
            detin_frame_letterboxed(a, f, src, sy + 1, sx, c0, n, padv, v10);
            detin_frame_letterboxed(a, f, src, sy + 1, sx + 1, c0, n, padv, v11);
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
