/*
 * evrep_oracle.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Plain-C, single-threaded restatement of the reference's event->tensor builders
 * and of its GWD score, used ONLY as the checker in tests/, in
 * __graft_entry__.smoke() and as bench.py's `cpu_baseline` ("port") leg.  Nothing
 * under event_representation_study_amd/ may import, link or call this file.
 *
 * Every function follows the reference's control flow (per-channel passes,
 * per-level puts, sequential scans) rather than the re-designed GPU data flow,
 * so it is an independent statement of the same arithmetic.  Citations are
 * relative to /root/reference.
 *
 * Pinning status (tests/test_oracle_golden.py compares against the npz files in tests/golden,
 * which were produced by importing the reference -- tests/golden/make_golden.py):
 *   A2  compute_repr            pinned, bit-exact
 *   A3-A5 MDES / ERGO-12        pinned bit-exact EXCEPT the torch_scatter.scatter
 *                               call boundary (package absent; semantics restated)
 *   A6  EventStack              pinned, bit-exact
 *   A7  TimeSurface             pinned, <= 1e-12 rel (libm exp vs numpy exp)
 *   A8  TORE                    pinned, <= 1e-6 rel (libm logf vs numpy f32 log)
 *   A9  GWD closed form         PARITY UNPINNED for POT's returned scalar (POT absent);
 *                               kernels/loss pinned by the import, <= 1e-5 rel
 *
 * Event layout everywhere: int32 rows [x, y, t, p], time-sorted ascending.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ORACLE_OK 0
#define ORACLE_EINDEX 1 /* an index the reference would raise IndexError on */
#define ORACLE_EARG 2

enum { F_TIMESTAMP = 0, F_POLARITY, F_COUNT, F_TIMESTAMP_POS, F_TIMESTAMP_NEG, F_COUNT_POS, F_COUNT_NEG };
enum { A_SUM = 0, A_MEAN, A_MAX, A_VARIANCE };

/* ---------------------------------------------------------------------------------------------
 * A3: the 7 "SBN" windows as [lo, hi) ranges of event rank
 * (mixed_density_event_stack.py:48-74).  w0 = all; w1..w3 = thirds of floor(N/3) (tail dropped);
 * w4..w6 = suffixes: a running count halves (N -> N//2 -> N//4 -> N//8) and is applied to the
 * already-sliced arrays, so the starts accumulate.
 * ------------------------------------------------------------------------------------------- */
void oracle_mdes_windows(int64_t n, int64_t lo[7], int64_t hi[7]) {
    int64_t third = n / 3;
    lo[0] = 0; hi[0] = n;
    for (int i = 0; i < 3; ++i) {
        lo[1 + i] = i * third < n ? i * third : n;
        hi[1 + i] = (i + 1) * third < n ? (i + 1) * third : n;
    }
    int64_t cur = n, start = 0;
    for (int i = 0; i < 3; ++i) {
        cur = cur / 2;
        start += cur;
        if (start > n) start = n;
        lo[4 + i] = start; hi[4 + i] = n;
    }
}

/* A4: one Operations(func, aggregation)(events[window]) call (operations.py:15-89) with the
 * torch_scatter semantics restated: sum accumulates sequentially in event order in float64;
 * mean = sum / max(count,1); max leaves empty pixels at 0; variance = mean(src^2) - mean(src)^2. */
static int mdes_channel(const int32_t *ev, const double *t_s, int64_t lo, int64_t hi, const unsigned char *mask, int H, int W,
                        int func, int agg, double *sum, double *sum2, double *cnt, double *chan /* H*W */) {
    /* mask != NULL ("SBT" stacking): the window is the events i in [lo, hi) with mask[i] set -- a boolean selection in array
     * order, as the reference's x[np.logical_and(...)] is */
    int64_t hw = (int64_t)H * W;
    int want = 0; /* 0 = all, +1 = p == 1, -1 = p == -1 (fallback p == 0) */
    if (func == F_TIMESTAMP_POS || func == F_COUNT_POS) want = 1;
    if (func == F_TIMESTAMP_NEG || func == F_COUNT_NEG) {
        want = -1;
        int any = 0;
        for (int64_t i = lo; i < hi; ++i) if ((!mask || mask[i]) && ev[4 * i + 3] == -1) { any = 1; break; }
        if (!any) want = -2; /* operations.py:59-61,78-80: no -1 rows -> use p == 0 rows */
    }
    /* index check first: torch scatter raises on any out-of-range index -> zero channel */
    for (int64_t i = lo; i < hi; ++i) {
        int p = ev[4 * i + 3];
        if (mask && !mask[i]) continue;
        if ((want == 1 && p != 1) || (want == -1 && p != -1) || (want == -2 && p != 0)) continue;
        int64_t idx = (int64_t)ev[4 * i] + (int64_t)ev[4 * i + 1] * W;
        if (idx < 0 || idx >= hw) return ORACLE_EINDEX;
    }
    memset(sum, 0, sizeof(double) * hw);
    memset(sum2, 0, sizeof(double) * hw);
    memset(cnt, 0, sizeof(double) * hw);
    int is_max = (agg == A_MAX);
    if (is_max) for (int64_t k = 0; k < hw; ++k) sum[k] = -1.7976931348623157e308;
    for (int64_t i = lo; i < hi; ++i) {
        int p = ev[4 * i + 3];
        if (mask && !mask[i]) continue;
        if ((want == 1 && p != 1) || (want == -1 && p != -1) || (want == -2 && p != 0)) continue;
        int64_t idx = (int64_t)ev[4 * i] + (int64_t)ev[4 * i + 1] * W;
        double v;
        switch (func) {
            case F_TIMESTAMP: case F_TIMESTAMP_POS: case F_TIMESTAMP_NEG: v = t_s[i]; break;
            case F_POLARITY: v = (double)p; break;
            default: v = 1.0; break;
        }
        if (is_max) { if (v > sum[idx] || v != v) sum[idx] = v; }
        else {
            sum[idx] += v;
            double v2 = v * v;
            sum2[idx] += v2;
        }
        cnt[idx] += 1.0;
    }
    for (int64_t k = 0; k < hw; ++k) {
        double c = cnt[k] < 1.0 ? 1.0 : cnt[k];
        switch (agg) {
            case A_SUM: chan[k] = sum[k]; break;
            case A_MEAN: chan[k] = sum[k] / c; break;
            case A_MAX: chan[k] = (sum[k] == -1.7976931348623157e308) ? 0.0 : sum[k]; break;
            default: {
                double m = sum[k] / c, m2 = sum2[k] / c;
                double mm = m * m;
                chan[k] = m2 - mm;
            }
        }
    }
    return ORACLE_OK;
}

/* A3/A5: MixedDensityEventStack.stack (mixed_density_event_stack.py:25-151).  out is (H, W, C)
 * float64.  win[c] < 0 or > 6 stands for the reference's `None` window -> zero channel
 * (any exception inside a channel -> zeros, :120-127). */
int oracle_mdes(const int32_t *ev, int64_t n, int H, int W, int C, const int *win, const int *func,
                const int *agg, double *out) {
    int64_t hw = (int64_t)H * W;
    if (n <= 0) return ORACLE_EARG; /* t.min() of an empty array raises in the reference */
    double *t_s = (double *)malloc(sizeof(double) * n);
    double *sum = (double *)malloc(sizeof(double) * hw), *sum2 = (double *)malloc(sizeof(double) * hw);
    double *cnt = (double *)malloc(sizeof(double) * hw), *chan = (double *)malloc(sizeof(double) * hw);
    int64_t tmin = ev[2], tmax = ev[2];
    for (int64_t i = 0; i < n; ++i) {
        int64_t t = ev[4 * i + 2];
        if (t < tmin) tmin = t;
        if (t > tmax) tmax = t;
    }
    double interval = (double)(tmax - tmin); /* :112-114, int64 / int64 -> float64 true divide */
    for (int64_t i = 0; i < n; ++i) t_s[i] = (double)((int64_t)ev[4 * i + 2] - tmin) / interval;
    int64_t lo[7], hi[7];
    oracle_mdes_windows(n, lo, hi);
    for (int c = 0; c < C; ++c) {
        int rc = ORACLE_EINDEX;
        if (win[c] >= 0 && win[c] <= 6 && func[c] >= 0 && func[c] <= 6 && agg[c] >= 0 && agg[c] <= 3)
            rc = mdes_channel(ev, t_s, lo[win[c]], hi[win[c]], NULL, H, W, func[c], agg[c], sum, sum2, cnt, chan);
        if (rc != ORACLE_OK) memset(chan, 0, sizeof(double) * hw);
        for (int64_t k = 0; k < hw; ++k) out[k * C + c] = chan[k];
    }
    free(t_s); free(sum); free(sum2); free(cnt); free(chan);
    return ORACLE_OK;
}

/* A3, stacking_type == "SBT" (mixed_density_event_stack.py:76-107): EIGHT windows cut by the normalised time t_s instead of
 * by event count.  w0 = all; w1..w3 = i/3 <= t_s <= (i+1)/3 (both ends inclusive, thresholds formed as python forms them:
 * equispaced_factor = 1/3, i * equispaced_factor); w4..w7 = t_s <= 1/2, 1/4, 1/8, 1/16 (each cut of the previous selection:
 * the same as the plain comparison).  Selections are boolean masks in array order.  mask_out (optional): [8][n]. */
int oracle_mdes_sbt(const int32_t *ev, int64_t n, int H, int W, int C, const int *win, const int *func,
                    const int *agg, double *out, unsigned char *mask_out) {
    int64_t hw = (int64_t)H * W;
    if (n <= 0) return ORACLE_EARG;
    double *t_s = (double *)malloc(sizeof(double) * n);
    double *sum = (double *)malloc(sizeof(double) * hw), *sum2 = (double *)malloc(sizeof(double) * hw);
    double *cnt = (double *)malloc(sizeof(double) * hw), *chan = (double *)malloc(sizeof(double) * hw);
    unsigned char *mask = (unsigned char *)malloc((size_t)8 * n);
    int64_t tmin = ev[2], tmax = ev[2];
    for (int64_t i = 0; i < n; ++i) {
        int64_t t = ev[4 * i + 2];
        if (t < tmin) tmin = t;
        if (t > tmax) tmax = t;
    }
    double interval = (double)(tmax - tmin);
    for (int64_t i = 0; i < n; ++i) t_s[i] = (double)((int64_t)ev[4 * i + 2] - tmin) / interval;
    const double ef = 1.0 / 3.0;
    for (int64_t i = 0; i < n; ++i) {
        mask[i] = 1;
        for (int k = 0; k < 3; ++k) mask[(size_t)(1 + k) * n + i] = (t_s[i] <= (double)(k + 1) * ef && t_s[i] >= (double)k * ef) ? 1 : 0;
        double factor = 1.0;
        for (int k = 0; k < 4; ++k) { factor = factor / 2.0; mask[(size_t)(4 + k) * n + i] = t_s[i] <= factor ? 1 : 0; }
    }
    for (int c = 0; c < C; ++c) {
        int rc = ORACLE_EINDEX;
        if (win[c] >= 0 && win[c] <= 7 && func[c] >= 0 && func[c] <= 6 && agg[c] >= 0 && agg[c] <= 3)
            rc = mdes_channel(ev, t_s, 0, n, mask + (size_t)win[c] * n, H, W, func[c], agg[c], sum, sum2, cnt, chan);
        if (rc != ORACLE_OK) memset(chan, 0, sizeof(double) * hw);
        for (int64_t k = 0; k < hw; ++k) out[k * C + c] = chan[k];
    }
    if (mask_out) memcpy(mask_out, mask, (size_t)8 * n);
    free(t_s); free(sum); free(sum2); free(cnt); free(chan); free(mask);
    return ORACLE_OK;
}

/* A5: the ERGO-12 triples (optimized_representation.py:86-115). */
static const int ERGO_WIN[12] = {0, 3, 2, 6, 5, 6, 2, 5, 1, 0, 4, 1};
static const int ERGO_FUNC[12] = {F_POLARITY, F_TIMESTAMP_NEG, F_COUNT_NEG, F_POLARITY, F_COUNT_POS, F_COUNT,
                                  F_TIMESTAMP_POS, F_COUNT_NEG, F_TIMESTAMP_NEG, F_TIMESTAMP_POS, F_TIMESTAMP, F_COUNT};
static const int ERGO_AGG[12] = {A_VARIANCE, A_VARIANCE, A_MEAN, A_SUM, A_MEAN, A_SUM,
                                 A_MEAN, A_MEAN, A_MAX, A_MAX, A_MAX, A_MEAN};

int oracle_ergo12(const int32_t *ev, int64_t n, int H, int W, double *out) {
    return oracle_mdes(ev, n, H, W, 12, ERGO_WIN, ERGO_FUNC, ERGO_AGG, out);
}

/* ---------------------------------------------------------------------------------------------
 * A6: EventStack.pre_stack + post_stack (event_stack.py:15-131) for time-sorted input with
 * last_timestamp = t[-1] (gen1_transforms.py:37-39), i.e. no "future" half.  `premap` applies
 * the dispatcher's p -> (p+1)//2 first (gen1_transforms.py:34).  Level k holds, per pixel, the
 * int8 polarity 2p-1 of the LAST event among events[off_k:], off_k = sum_{j<=k} N // 2^j
 * (ndarray.put is last-write-wins, :125; the delta encode / re-accumulate of :88-114 / :45-63
 * reproduces exactly the per-level image).  out is (H, W, S) float32.
 * ------------------------------------------------------------------------------------------- */
int oracle_event_stack(const int32_t *ev, int64_t n, int H, int W, int S, int premap, float *out) {
    int64_t hw = (int64_t)H * W;
    if (n <= 0) return ORACLE_EARG;
    int8_t *img = (int8_t *)malloc(hw);
    int64_t cur = n, off = 0;
    for (int k = 0; k < S; ++k) {
        memset(img, 0, hw);
        for (int64_t i = off; i < n; ++i) {
            int64_t idx = (int64_t)ev[4 * i + 1] * W + ev[4 * i];
            if (idx < -hw || idx >= hw) { free(img); return ORACLE_EINDEX; }
            if (idx < 0) idx += hw; /* numpy put wraps negative indices in 'raise' mode */
            int p = ev[4 * i + 3];
            if (premap == 1) p = (p + 1) >> 1; /* floor division by 2 */
            /* premap 2: the column already holds the int8 value 2p-1 (or its negation, the future half, :35) */
            img[idx] = (int8_t)(premap == 2 ? p : 2 * p - 1);
        }
        for (int64_t q = 0; q < hw; ++q) out[q * S + k] = (float)img[q];
        cur = cur / 2;
        off += cur;
    }
    free(img);
    return ORACLE_OK;
}

/* ---------------------------------------------------------------------------------------------
 * A7: ToTimesurface.__call__ + to_timesurface_numpy (time_surface.py:25-74) driven as
 * gen1_transforms.py:69-85 does: p -> ((p+1)/2) truncated to {0,1}; idx = searchsorted(t_norm,
 * 1..6, 'left') with t_norm = (t - t0) / (t_last - t0) * 6 in float64.  One sequential scan;
 * when i == idx[s] the whole (2,H,W) memory is turned into exp((mem - t_i)/tau) and s advances
 * (an `if`, not a `while`: equal consecutive idx leave every later slice all-zero).
 * out is (H, W, 2*S) float64 with channel c = 2*s + p.   idx_out (S entries) may be NULL.
 * ------------------------------------------------------------------------------------------- */
int oracle_time_surface(const int32_t *ev, int64_t n, int H, int W, int S, double tau, int premap,
                        int64_t *idx_out, double *out) {
    int64_t hw = (int64_t)H * W;
    if (n <= 0 || S <= 0 || S > 64) return ORACLE_EARG;
    int64_t idx[64];
    int32_t t0 = ev[2], tl = ev[4 * (n - 1) + 2];
    for (int s = 0; s < S; ++s) { /* np.searchsorted(..., side='left') as a binary search */
        double target = (double)(s + 1);
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            int64_t mid = lo + (hi - lo) / 2;
            double tn = (double)(int32_t)(ev[4 * mid + 2] - t0) / (double)(int32_t)(tl - t0) * (double)S;
            if (tn < target) lo = mid + 1; else hi = mid;
        }
        idx[s] = lo;
        if (idx_out) idx_out[s] = lo;
    }
    double *mem = (double *)malloc(sizeof(double) * 2 * hw);
    for (int64_t k = 0; k < 2 * hw; ++k) mem[k] = -(tau * 3 + 1);
    memset(out, 0, sizeof(double) * hw * 2 * S);
    int s = 0;
    for (int64_t i = 0; i < n; ++i) {
        int p = ev[4 * i + 3];
        if (premap) p = (int)(int8_t)((double)(p + 1) / 2.0); /* astype(int8) truncates toward zero */
        int x = ev[4 * i], y = ev[4 * i + 1];
        if (p < -2 || p >= 2 || y < -H || y >= H || x < -W || x >= W) { free(mem); return ORACLE_EINDEX; }
        if (p < 0) p += 2;
        if (y < 0) y += H;
        if (x < 0) x += W;
        mem[(int64_t)p * hw + (int64_t)y * W + x] = (double)ev[4 * i + 2];
        if (i == idx[s]) {
            double ti = (double)ev[4 * i + 2];
            for (int pp = 0; pp < 2; ++pp)
                for (int64_t q = 0; q < hw; ++q)
                    out[q * 2 * S + 2 * s + pp] = exp((mem[(int64_t)pp * hw + q] - ti) / tau);
            if (++s > S - 1) break;
        }
    }
    free(mem);
    return ORACLE_OK;
}

/* ---------------------------------------------------------------------------------------------
 * A8: events2ToreFeature (tore.py:6-83) for a single sample time T.  x, y are the 1-based
 * coordinates the caller built (gen1_transforms.py:61-64); pixel = [y-1, x-1] in a (Hf, Wf) frame.
 * Events with ts >= T are excluded (:17).  Per pixel and polarity (pol > 0 / pol <= 0) a k-vector v of dt = T - ts,
 * +inf when missing; every event, in ARRAY order, replaces it by np.partition([dt] + v[:k-1], k-1)[:k] (:22-47).
 * numpy's float64 partition of so short a vector returns it SORTED (numpy >= 2.0 on AVX2 / AVX-512 hosts dispatches to
 * x86-simd-sort, whose qselect runs a bitonic sorting network on arrays of <= 256 elements; pinned by
 * tests/golden/tore_unsorted_*.npz, generated here with numpy 2.2.6 on an AVX-512 host), so a step inserts dt into the
 * ascending k - 1 smallest kept so far, and the largest of the k is dropped by the pixel's NEXT event.  (The scalar
 * introselect of other numpy builds only swaps the maximum to the end: the same values in another order whenever the
 * timestamps are not ascending.)  On time-sorted input every new dt is the smallest: a k-deep FIFO, newest first.
 * Then float32: clamp to 5e8, log(v+1) - log(151), floor 0 (a NaN, from a wrapped dt <= -2, stays NaN).
 * out is (Hf, Wf, 2k) float32: pos[0..k), neg[0..k).
 * ------------------------------------------------------------------------------------------- */
int oracle_tore(const int32_t *x, const int32_t *y, const int32_t *ts, const int32_t *pol, int64_t n,
                double T, int k, int Hf, int Wf, float *out) {
    int64_t hw = (int64_t)Hf * Wf;
    if (k <= 0 || Hf <= 0 || Wf <= 0) return ORACLE_EARG;
    double *fifo = (double *)malloc(sizeof(double) * hw * 2 * k);
    for (int64_t q = 0; q < hw * 2 * k; ++q) fifo[q] = INFINITY;
    /* an int32 sample time (the dispatcher's ts[-1], an np.int32) minus the int32 ts array is int32 arithmetic in numpy
     * (tore.py:20,35): T - ts wraps past INT32_MAX, to a negative dt that sorts first and whose log is NaN */
    const int int32_T = T == floor(T) && T >= (double)INT32_MIN && T <= (double)INT32_MAX;
    for (int pass = 0; pass < 2; ++pass) { /* the reference handles all positives, then all negatives */
        for (int64_t i = 0; i < n; ++i) {
            if (!((double)ts[i] < T)) continue;
            int is_pos = pol[i] > 0;
            if (is_pos != (pass == 0)) continue;
            int64_t r = (int64_t)y[i] - 1, c = (int64_t)x[i] - 1;
            if (r < -Hf || r >= Hf || c < -Wf || c >= Wf) { free(fifo); return ORACLE_EINDEX; }
            if (r < 0) r += Hf; /* numpy negative-index wrap */
            if (c < 0) c += Wf;
            double *f = fifo + ((r * Wf + c) * 2 + (is_pos ? 0 : 1)) * k;
            /* w = [dt] + f[:k-1], sorted ascending (insertion of dt into the sorted k - 1 kept values) */
            double dt = int32_T ? (double)(int32_t)(uint32_t)((int64_t)T - (int64_t)ts[i]) : T - (double)ts[i];
            int j = k - 1;
            while (j > 0 && f[j - 1] > dt) { f[j] = f[j - 1]; --j; }
            f[j] = dt;
        }
    }
    const double log_min = log(150.0 + 1.0);
    for (int64_t q = 0; q < hw * 2 * k; ++q) {
        float v = (float)fifo[q]; /* .astype(np.float32) */
        if (v != v) v = 500e6f;
        if (v > 500e6f) v = 500e6f;
        float l = logf(v + 1.0f);
        float r = (float)((double)l - log_min); /* numpy 2 (NEP 50): f32 array -= f64 scalar runs in f64 */
        if (r < 0.0f) r = 0.0f;
        out[q] = r;
    }
    free(fifo);
    return ORACLE_OK;
}

/* A8 as the dispatcher drives it (gen1_transforms.py:51-66): origin-shift to the events'
 * bounding box, frame = (max y', max x'), T = ts[-1].  Call with out == NULL to get the frame. */
int oracle_tore_bbox(const int32_t *ev, int64_t n, int k, int *Hf, int *Wf, float *out) {
    if (n <= 0) return ORACLE_EARG;
    int32_t xmin = ev[0], xmax = ev[0], ymin = ev[1], ymax = ev[1];
    for (int64_t i = 0; i < n; ++i) {
        if (ev[4 * i] < xmin) xmin = ev[4 * i];
        if (ev[4 * i] > xmax) xmax = ev[4 * i];
        if (ev[4 * i + 1] < ymin) ymin = ev[4 * i + 1];
        if (ev[4 * i + 1] > ymax) ymax = ev[4 * i + 1];
    }
    *Hf = ymax - ymin + 1;
    *Wf = xmax - xmin + 1;
    if (!out) return ORACLE_OK;
    int32_t *buf = (int32_t *)malloc(sizeof(int32_t) * 4 * n);
    int32_t *x = buf, *y = buf + n, *t = buf + 2 * n, *p = buf + 3 * n;
    for (int64_t i = 0; i < n; ++i) {
        x[i] = ev[4 * i] - xmin + 1; y[i] = ev[4 * i + 1] - ymin + 1;
        t[i] = ev[4 * i + 2]; p[i] = ev[4 * i + 3];
    }
    int rc = oracle_tore(x, y, t, p, n, (double)t[n - 1], k, *Hf, *Wf, out);
    free(buf);
    return rc;
}

/* ---------------------------------------------------------------------------------------------
 * A2: compute_repr (representation_search/gromov_wasserstein.py:72-82), the in-repo voxel grid,
 * with the caller's normalisation t = (t - t[0]) / (t[-1] - t[0]) (:96).  Two np.add.at passes
 * (lower bin for every event, then upper bin for every event), float64, event order.
 * out is (H, W, bins) float64.
 * ------------------------------------------------------------------------------------------- */
int oracle_voxel(const int32_t *ev, int64_t n, int H, int W, int bins, double *out) {
    int64_t hw = (int64_t)H * W;
    if (n <= 0 || bins <= 0) return ORACLE_EARG;
    memset(out, 0, sizeof(double) * hw * bins);
    double t0 = (double)ev[2], tl = (double)ev[4 * (n - 1) + 2];
    for (int pass = 0; pass < 2; ++pass) {
        for (int64_t i = 0; i < n; ++i) {
            double tn = ((double)ev[4 * i + 2] - t0) / (tl - t0);
            double b = (double)(bins - 1) * tn;
            int64_t blim = (int64_t)b + pass;
            if (!(blim < bins)) continue;
            double w = 1.0 - fabs((double)blim - b);
            int x = ev[4 * i], y = ev[4 * i + 1];
            if (y < -H || y >= H || x < -W || x >= W || blim < -bins) return ORACLE_EINDEX;
            if (y < 0) y += H;
            if (x < 0) x += W;
            if (blim < 0) blim += bins;
            double wp = w * (double)ev[4 * i + 3];
            out[((int64_t)y * W + x) * bins + blim] += wp;
        }
    }
    return ORACLE_OK;
}

/* ---------------------------------------------------------------------------------------------
 * F3: ev-licious events_to_voxel_grid, numpy variant, integer pixels, no normalisation
 * (ev-licious/src/evlicious/tools/utils.py:52-76,100-108).  t_norm = (bins-1)*(t-t0)/deltaT in
 * float64; both tlim in {int(t_norm), int(t_norm)+1} are drawn with weight (1 - |tlim - int(t_norm)|)*p,
 * i.e. p and 0, accumulated with np.add.at into a float32 grid.  out is (bins, H, W) float32.
 * ------------------------------------------------------------------------------------------- */
int oracle_evl_voxel_range(const int32_t *ev, int64_t n, int H, int W, int bins, int has_t0, int64_t t0_us,
                           int has_t1, int64_t t1_us, float *out);
int oracle_evl_voxel(const int32_t *ev, int64_t n, int H, int W, int bins, float *out) {
    return oracle_evl_voxel_range(ev, n, H, W, bins, 0, 0, 0, 0, out);
}
/* the same with the optional t0_us / t1_us arguments (utils.py:60-63); events outside the range get a bin index
 * outside [0, bins) and are masked (:69), except that astype("int32") truncates toward zero (:67) */
int oracle_evl_voxel_range(const int32_t *ev, int64_t n, int H, int W, int bins, int has_t0, int64_t t0_us,
                           int has_t1, int64_t t1_us, float *out) {
    int64_t hw = (int64_t)H * W;
    memset(out, 0, sizeof(float) * hw * bins);
    if (n < 2) return ORACLE_OK;
    int64_t t0 = has_t0 ? t0_us : ev[2], t1 = has_t1 ? t1_us : ev[4 * (n - 1) + 2];
    double deltaT = (double)(t1 - t0);
    if (t1 - t0 == 0) deltaT = 1.0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int64_t i = 0; i < n; ++i) {
            double tn = (double)((int64_t)(bins - 1) * ((int64_t)ev[4 * i + 2] - t0)) / deltaT;
            int32_t ti = (int32_t)tn;
            int32_t tlim = ti + pass;
            if (!(tlim >= 0 && tlim < bins)) continue;
            int32_t wgt = (1 - abs(tlim - ti)) * ev[4 * i + 3];
            int x = ev[4 * i], y = ev[4 * i + 1];
            if (!(x >= 0 && y >= 0 && x < W && y < H)) continue; /* _draw_xy_to_voxel_grid_int masks these */
            out[(int64_t)tlim * hw + (int64_t)y * W + x] += (float)wgt;
        }
    }
    return ORACLE_OK;
}

/* ---------------------------------------------------------------------------------------------
 * A9: OTMI.__init__/loss/solve (compute_otmi.py:61-93) in the closed form SURVEY.md section 8 A9
 * derives for POT's max_iter=0 path: C = mean over the L x L zero-padded grid of |Ks - Kt|,
 * L = max(n, m), Ks = exp(-(Cs/(h*sig_s))^2 / 2), sig = sqrt(mean(C^2)/2), C = pairwise L2.
 * The reference carries Ks in float32 (Xs is float32); this oracle works in float64 throughout,
 * a <= 1e-6 relative difference.  Xs is (n, ds) row-major, Xt is (m, dt).  O((n^2+m^2) d).
 * ------------------------------------------------------------------------------------------- */
static double sq_dist(const double *a, const double *b, int d) {
    double s = 0.0;
    for (int k = 0; k < d; ++k) { double u = a[k] - b[k]; s += u * u; }
    return s;
}

static double mean_sq_dist(const double *X, int64_t n, int d) {
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        double r = 0.0;
        for (int64_t j = 0; j < n; ++j) r += sq_dist(X + i * d, X + j * d, d);
        s += r;
    }
    return s / ((double)n * (double)n);
}

int oracle_gwd(const double *Xs, int64_t n, int ds, const double *Xt, int64_t m, int dt, double h,
               double *cost) {
    if (n <= 0 || m <= 0) return ORACLE_EARG;
    double sig_s = sqrt(mean_sq_dist(Xs, n, ds) / 2.0), sig_t = sqrt(mean_sq_dist(Xt, m, dt) / 2.0);
    double hs = h * sig_s, ht = h * sig_t;
    int64_t L = n > m ? n : m;
    double total = 0.0;
    for (int64_t i = 0; i < L; ++i) {
        double row = 0.0;
        for (int64_t j = 0; j < L; ++j) {
            double ks = 0.0, kt = 0.0;
            if (i < n && j < n) { double c = sqrt(sq_dist(Xs + i * ds, Xs + j * ds, ds)) / hs; ks = exp(-(c * c) / 2.0); }
            if (i < m && j < m) { double c = sqrt(sq_dist(Xt + i * dt, Xt + j * dt, dt)) / ht; kt = exp(-(c * c) / 2.0); }
            row += fabs(ks - kt);
        }
        total += row;
    }
    *cost = total / ((double)L * (double)L);
    return ORACLE_OK;
}
