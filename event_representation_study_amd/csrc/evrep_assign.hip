// evrep_assign.hip -- the training targets: what ev-YOLOv6's ComputeLoss.__call__ does between the head's output and the loss
// terms (yolov6/models/losses/loss.py:73-111): ComputeLoss.preprocess (loss.py:219-236) and TaskAlignedAssigner.forward
// (yolov6/assigners/tal_assigner.py with assigner_utils.py) for the B images of a batch, with no (B, M, A) array in memory.
// include/evrep.h states the rules with evrep_det_targets_pad and evrep_tal_assign.
//
//   k_det_targets_pad  one workgroup of sixteen waves per image lists its label rows in array order (the scan of evrep_deteval.hip),
//                      writes [cls, x1, y1, x2, y2] in float64 for the first M of them and [-1, 0, 0, 0, 0] behind them.
//   k_tal_prepare      grid (G, B): every value of the image's predictions and labels is looked at once; a non-finite one sets
//                      EVREP_TAL_ST_NONFINITE in status[b].  Clears the per-anchor words and the per-row maxima of the scratch.
//   k_tal_select       one workgroup per (image, row).  A valid row streams the A anchors in chunks of 256, a lane per anchor,
//                      and keeps the first `topk` of the total order (key descending, anchor ascending) in LDS (TopkList below).
//                      Every selected anchor whose centre lies in the box adds 1 to cnt[b, a] and takes min(first[b, a], m):
//                      integer atomics, free of order.
//   k_tal_resolve      a lane per (image, anchor): c = cnt; the row is first (c == 1) or the first row of greatest IoU over all M
//                      rows (c > 1); writes the label, the box, fg, and keeps the row and its metric in the scratch; folds the
//                      metric and the IoU into the row's maxima with a 64-bit integer atomicMax on the bit patterns (only
//                      positive values take part: they order as their bits).
//   k_tal_scores       a lane per element of target_scores: zero, or (al * pos_ov) / (pos_al + 1e-9) at a foreground anchor's label.
//
// ROUNDING.  Every statement is one operation of the type evrep.h states, written with __dadd_rn / __dsub_rn / __dmul_rn /
// __ddiv_rn (and __fsub_rn / __fmul_rn for the one float32 quantity, the predicted box's area); the library is compiled with
// -ffp-contract=off and this file repeats it as a pragma.  max(a, b) is a > b ? a : b and min(a, b) is a < b ? a : b.
//
// Every loop ends at a value the host passed; every index is below the size the host stated.  Plain C++ stores, integer
// atomics only, nothing read back, no allocation: the launches can be captured into a graph.
#pragma once
#include "evrep_common.h"
#include "evrep_ranksort.h"

#pragma clang fp contract(off)

namespace evrep {

constexpr int kTalMaxTopk = EVREP_TAL_MAX_TOPK;
constexpr int kTalSelectThreads = 256;                                 // k_tal_select: a chunk of anchors, a lane each

struct TalPadArgs {
    const float *targets;         // (n_t, 6)
    double *gt;                   // (B, M, 5)
    int32_t *n_labels;            // (B)
    uint32_t *status;             // (B)
    int64_t n_t;
    double W, H;
    int32_t B, M;
};

struct TalArgs {
    const float *pd_scores;       // (B, A, nc)
    const float *pd_bboxes;       // (B, A, 4)
    const float *anc;             // (A, 2)
    const double *gt;             // (B, M, 5)
    int64_t *labels;              // (B, A)
    void *boxes;                  // (B, A, 4) double or float
    void *scores;                 // (B, A, nc) double or float
    uint8_t *fg;                  // (B, A)
    uint32_t *status;             // (B)
    uint32_t *cnt;                // scratch (B, A): the rows an anchor is a candidate of
    uint32_t *first;              // scratch (B, A): the lowest of them
    int32_t *row;                 // scratch (B, A): the assigned row, -1 for background
    double *val;                  // scratch (B, A): the assigned row's metric
    unsigned long long *pos_al;   // scratch (B, M): bits of the row's greatest metric
    unsigned long long *pos_ov;   // scratch (B, M): bits of the row's greatest IoU
    int32_t B, M, A, nc, topk, alpha, beta, f32_out;
};

__device__ inline bool tal_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ inline bool tal_finite(double v) {
    return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
__device__ inline double tal_max(double a, double b) { return a > b ? a : b; }
__device__ inline double tal_min(double a, double b) { return a < b ? a : b; }

// x^n by n - 1 multiplications, left to right; x^0 = 1
__device__ inline double tal_pow(double x, int n) {
    if (n == 0) return 1.0;
    double r = x;
    for (int i = 1; i < n; ++i) r = __dmul_rn(r, x);
    return r;
}

struct TalRow {
    double cls, x1, y1, x2, y2;
};

__device__ inline TalRow tal_row(const double *gt, int b, int M, int m) {
    const double *g = gt + ((size_t)b * (size_t)M + (size_t)m) * 5u;   // m < M
    TalRow r;
    r.cls = g[0]; r.x1 = g[1]; r.y1 = g[2]; r.x2 = g[3]; r.y2 = g[4];
    return r;
}

// mask_gt: ((x1 + y1) + x2) + y2 > 0
__device__ inline bool tal_row_valid(const TalRow &r) { return __dadd_rn(__dadd_rn(__dadd_rn(r.x1, r.y1), r.x2), r.y2) > 0.0; }
// long(cls) when it lies in [0, nc), else -1
__device__ inline int tal_class(double c, int nc) { return (c >= 0.0 && c < (double)nc) ? (int)c : -1; }

__device__ inline bool tal_in_gt(const TalRow &r, double ax, double ay) {
    const double d = tal_min(tal_min(__dsub_rn(ax, r.x1), __dsub_rn(ay, r.y1)), tal_min(__dsub_rn(r.x2, ax), __dsub_rn(r.y2, ay)));
    return d > 1e-9;
}

// iou_calculator(gt box, predicted box): float64 but for the predicted box's own area
__device__ inline double tal_iou(const TalRow &r, const float4 p) {
    const double px1 = (double)p.x, py1 = (double)p.y, px2 = (double)p.z, py2 = (double)p.w;
    const double ix1 = tal_max(r.x1, px1), iy1 = tal_max(r.y1, py1), ix2 = tal_min(r.x2, px2), iy2 = tal_min(r.y2, py2);
    const double ov = __dmul_rn(tal_max(__dsub_rn(ix2, ix1), 0.0), tal_max(__dsub_rn(iy2, iy1), 0.0));
    const double a1 = __dmul_rn(tal_max(__dsub_rn(r.x2, r.x1), 0.0), tal_max(__dsub_rn(r.y2, r.y1), 0.0));
    const float w = __fsub_rn(p.z, p.x), h = __fsub_rn(p.w, p.y);
    const double a2 = (double)__fmul_rn(w > 0.0f ? w : 0.0f, h > 0.0f ? h : 0.0f);
    return __ddiv_rn(ov, __dadd_rn(__dsub_rn(__dadd_rn(a1, a2), ov), 1e-9));
}

__device__ inline float4 tal_pbox(const float *pd_bboxes, int b, int A, int a) {
    const float *p = pd_bboxes + ((size_t)b * (size_t)A + (size_t)a) * 4u;   // a < A
    return make_float4(p[0], p[1], p[2], p[3]);
}

// score^alpha * iou^beta of class `cl` in [0, nc)
__device__ inline double tal_metric(const TalArgs &t, int b, int a, int cl, double iou) {
    const double s = (double)t.pd_scores[((size_t)b * (size_t)t.A + (size_t)a) * (size_t)t.nc + (size_t)cl];
    return __dmul_rn(tal_pow(s, t.alpha), tal_pow(iou, t.beta));
}

// ---------------------------------------------------------------------------------------------------------------- preprocess
// grid (B), 1024 threads
__global__ __launch_bounds__(kDistThreads) void k_det_targets_pad(const TalPadArgs a) {
    __shared__ uint32_t s_scan[kDistWaves];
    const int tid = threadIdx.x, b = blockIdx.x, M = a.M;
    const float fb = (float)b;
    double *gt = a.gt + (size_t)b * (size_t)M * 5u;
    uint32_t n = 0;
    for (int64_t r0 = 0; r0 < a.n_t; r0 += kDistThreads) {
        const int64_t r = r0 + tid;
        const bool in = r < a.n_t;
        const float *t = a.targets + (size_t)(in ? r : 0) * 6u;
        const bool mine = in && t[0] == fb;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<kDistWaves>(mine ? 1u : 0u, s_scan, &tot);
        const uint32_t pos = n + ex;
        if (mine && pos < (uint32_t)M) {
            const double bx = __dmul_rn((double)t[2], a.W), by = __dmul_rn((double)t[3], a.H);
            const double bw = __dmul_rn((double)t[4], a.W), bh = __dmul_rn((double)t[5], a.H);
            const double x1 = __dsub_rn(bx, __dmul_rn(bw, 0.5)), y1 = __dsub_rn(by, __dmul_rn(bh, 0.5));
            double *o = gt + (size_t)pos * 5u;                          // pos < M
            gstore_f64(o + 0, (double)t[1]);
            gstore_f64(o + 1, x1);
            gstore_f64(o + 2, y1);
            gstore_f64(o + 3, __dadd_rn(x1, bw));
            gstore_f64(o + 4, __dadd_rn(y1, bh));
        }
        n += tot;
    }
    for (int m = (n < (uint32_t)M ? (int)n : M) + tid; m < M; m += kDistThreads) {
        double *o = gt + (size_t)m * 5u;
        gstore_f64(o + 0, -1.0);
        gstore_f64(o + 1, 0.0); gstore_f64(o + 2, 0.0); gstore_f64(o + 3, 0.0); gstore_f64(o + 4, 0.0);
    }
    if (tid == 0) {
        a.n_labels[b] = (int32_t)n;
        a.status[b] = n > (uint32_t)M ? EVREP_TAL_ST_LABEL_OVERFLOW : 0u;
    }
}

// ------------------------------------------------------------------------------------------------------------------- prepare
// The pieces both assigners' prepare kernels are made of.  A non-finite value among ptr[start], ptr[start + step], ... below n:
template <typename T>
__device__ inline bool any_nonfinite(const T *ptr, size_t n, size_t start, size_t step) {
    bool bad = false;
    for (size_t e = start; e < n; e += step) bad = bad || !tal_finite(ptr[e]);
    return bad;
}

// the claim words of image b's anchors: claimed by no row
__device__ inline void claims_clear(uint32_t *cnt, uint32_t *first, int b, int A, size_t start, size_t step) {
    for (size_t a = start; a < (size_t)A; a += step) {
        cnt[(size_t)b * A + a] = 0u;
        first[(size_t)b * A + a] = 0xFFFFFFFFu;
    }
}

// EVREP_TAL_ST_NONFINITE into *status where a lane of the workgroup found a bad value.  Holds an LDS word and two barriers:
// every lane of the workgroup calls it, outside divergent control flow.
__device__ inline void raise_nonfinite(bool bad, uint32_t *status) {
    __shared__ uint32_t s_bad;
    if (threadIdx.x == 0) s_bad = 0u;
    __syncthreads();
    if (bad) s_bad = 1u;
    __syncthreads();
    if (threadIdx.x == 0 && s_bad != 0u) atomicOr(status, EVREP_TAL_ST_NONFINITE);
}

// grid (G, B), 256 threads; status[b] was zeroed by a memset ordered before this launch
__global__ __launch_bounds__(kThreads) void k_tal_prepare(const TalArgs t) {
    const int b = blockIdx.y;
    const size_t start = (size_t)blockIdx.x * kThreads + threadIdx.x, step = (size_t)gridDim.x * kThreads;
    const size_t n_s = (size_t)t.A * (size_t)t.nc, n_b = (size_t)t.A * 4u, n_g = (size_t)t.M * 5u;
    bool bad = any_nonfinite(t.pd_scores + (size_t)b * n_s, n_s, start, step);
    bad = bad || any_nonfinite(t.pd_bboxes + (size_t)b * n_b, n_b, start, step);
    bad = bad || any_nonfinite(t.gt + (size_t)b * n_g, n_g, start, step);
    claims_clear(t.cnt, t.first, b, t.A, start, step);
    for (size_t m = start; m < (size_t)t.M; m += step) {
        t.pos_al[(size_t)b * t.M + m] = 0ull;
        t.pos_ov[(size_t)b * t.M + m] = 0ull;
    }
    raise_nonfinite(bad, &t.status[b]);
}

// ------------------------------------------------------------------------------------------------------------ the top-k list
// The first K <= MaxK entries of a total order, kept in LDS by a workgroup of Threads lanes that is offered its entries a
// chunk at a time, a lane each.  An entry is the bits of a key and an index; Before(k1, i1, k2, i2) says that entry 1 comes
// before entry 2, and no two entries offered are equal.  A chunk's entries that come before the list's last one are appended
// behind the list; every entry is then ranked by counting the entries before it, and the first K are the new list.
// Storage lies in LDS; the list itself (K and the length, equal in every lane) lives in registers.
template <int MaxK, int Threads, typename Before>
class TopkList {
    static_assert(MaxK <= Threads, "the list is merged by the lanes of one chunk");

public:
    struct Storage {
        unsigned long long k[MaxK + Threads], nk[MaxK];
        uint32_t i[MaxK + Threads], ni[MaxK];
        uint32_t scan[Threads / 64];
    };

    __device__ TopkList(Storage &s, int K) : s_(s), K_(K), L_(0) {}   // 1 <= K <= MaxK

    // Every lane of the workgroup calls, `in` or not: the lane's entry of this chunk.
    __device__ void offer(bool in, unsigned long long kb, uint32_t ib) {
        const int tid = threadIdx.x, K = K_, L = L_;
        const Before before;
        // the list's last entry is read before anyone rewrites it: the barriers of the scan stand between
        const bool cont = in && (L < K || before(kb, ib, s_.k[L - 1], s_.i[L - 1]));
        uint32_t nc_;
        const uint32_t ex = block_exclusive_scan<Threads / 64>(cont ? 1u : 0u, s_.scan, &nc_);
        if (nc_ == 0u) return;                                         // (uniform)
        if (cont) {
            s_.k[L + ex] = kb;                                         // L + ex < K + Threads
            s_.i[L + ex] = ib;
        }
        __syncthreads();
        const int T = L + (int)nc_;
        const int NL = T < K ? T : K;
        for (int e = tid; e < T; e += Threads) {
            const unsigned long long ke = s_.k[e];
            const uint32_t ie = s_.i[e];
            int rank = 0;
            for (int j = 0; j < T; ++j) rank += before(s_.k[j], s_.i[j], ke, ie) ? 1 : 0;
            if (rank < NL) {                                           // the entries are distinct: so are the ranks
                s_.nk[rank] = ke;
                s_.ni[rank] = ie;
            }
        }
        __syncthreads();
        if (tid < NL) {
            s_.k[tid] = s_.nk[tid];
            s_.i[tid] = s_.ni[tid];
        }
        L_ = NL;
        __syncthreads();
    }

    __device__ int size() const { return L_; }                         // <= min(K, entries offered)
    __device__ uint32_t index(int e) const { return s_.i[e]; }         // e < size(), in the order

private:
    Storage &s_;
    const int K_;
    int L_;
};

// -------------------------------------------------------------------------------------------------------------------- select
// an entry of the order: the key's bits (non-negative doubles order as their bits) and A - 1 - anchor
struct TalAbove {
    __device__ bool operator()(unsigned long long k1, uint32_t i1, unsigned long long k2, uint32_t i2) const {
        return k1 > k2 || (k1 == k2 && i1 > i2);
    }
};
using TalList = TopkList<kTalMaxTopk, kTalSelectThreads, TalAbove>;

// grid (M, B), 256 threads
__global__ __launch_bounds__(kTalSelectThreads) void k_tal_select(const TalArgs t) {
    __shared__ TalList::Storage s_list;
    const int tid = threadIdx.x, m = blockIdx.x, b = blockIdx.y, A = t.A;
    if (t.status[b] & EVREP_TAL_ST_NONFINITE) return;                   // (uniform: written by the launch before this one)
    const TalRow r = tal_row(t.gt, b, t.M, m);
    if (!tal_row_valid(r)) return;
    const int cl = tal_class(r.cls, t.nc);
    if (cl < 0) {
        if (tid == 0) atomicOr(&t.status[b], EVREP_TAL_ST_BAD_CLASS);
        return;
    }
    TalList list(s_list, t.topk);
    for (int a0 = 0; a0 < A; a0 += kTalSelectThreads) {
        const int a = a0 + tid;
        unsigned long long kb = 0ull;
        if (a < A) {
            const double ax = (double)t.anc[(size_t)a * 2u], ay = (double)t.anc[(size_t)a * 2u + 1u];
            if (tal_in_gt(r, ax, ay)) {
                const double al = tal_metric(t, b, a, cl, tal_iou(r, tal_pbox(t.pd_bboxes, b, A, a)));
                if (al > 0.0) kb = (unsigned long long)__double_as_longlong(al);   // (a NaN, a negative and -0 are key +0)
            }
        }
        list.offer(a < A, kb, (uint32_t)(A - 1 - (a < A ? a : A - 1)));
    }
    if (tid < list.size()) {
        const int a = A - 1 - (int)list.index(tid);                    // 0 <= a < A
        const double ax = (double)t.anc[(size_t)a * 2u], ay = (double)t.anc[(size_t)a * 2u + 1u];
        if (tal_in_gt(r, ax, ay)) {
            atomicAdd(&t.cnt[(size_t)b * A + a], 1u);
            atomicMin(&t.first[(size_t)b * A + a], (uint32_t)m);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- resolve
// base[at] = v in the output's width: float32 (one rounding) or float64
__device__ inline void tal_store(void *base, int f32, size_t at, double v) {
    if (f32) static_cast<float *>(base)[at] = (float)v;
    else static_cast<double *>(base)[at] = v;
}

// grid (ceil(A / 256), B), 256 threads.  M == 0: the reference's early return
__global__ __launch_bounds__(kThreads) void k_tal_resolve(const TalArgs t) {
    const int b = blockIdx.y, a = blockIdx.x * kThreads + threadIdx.x, A = t.A, M = t.M;
    if (a >= A) return;
    const size_t ba = (size_t)b * A + a;
    if (M == 0) {
        t.labels[ba] = (int64_t)t.nc;
        t.fg[ba] = 0;
        t.row[ba] = -1;
        t.val[ba] = 0.0;
        for (int e = 0; e < 4; ++e) tal_store(t.boxes, t.f32_out, ba * 4u + e, 0.0);
        return;
    }
    const uint32_t c = t.cnt[ba];
    int g = 0;
    double iou = 0.0, al = 0.0;
    if (c != 0u) {
        const float4 p = tal_pbox(t.pd_bboxes, b, A, a);
        if (c == 1u) {
            g = (int)t.first[ba];                                      // a row that claimed the anchor: < M
            iou = tal_iou(tal_row(t.gt, b, M, g), p);
        } else {
            iou = tal_iou(tal_row(t.gt, b, M, 0), p);
            for (int m = 1; m < M; ++m) {
                const double v = tal_iou(tal_row(t.gt, b, M, m), p);
                if (v > iou) {
                    iou = v;
                    g = m;
                }
            }
        }
    }
    const TalRow r = tal_row(t.gt, b, M, g);
    const int cl = tal_class(r.cls, t.nc);
    if (c != 0u) {
        al = cl >= 0 ? tal_metric(t, b, a, cl, iou) : 0.0;
        if (al > 0.0) atomicMax(&t.pos_al[(size_t)b * M + g], (unsigned long long)__double_as_longlong(al));
        if (iou > 0.0) atomicMax(&t.pos_ov[(size_t)b * M + g], (unsigned long long)__double_as_longlong(iou));
    }
    t.labels[ba] = (int64_t)(cl < 0 ? 0 : cl);
    t.fg[ba] = c != 0u ? 1 : 0;
    t.row[ba] = c != 0u ? g : -1;
    t.val[ba] = al;
    const double box[4] = {r.x1, r.y1, r.x2, r.y2};
    for (int e = 0; e < 4; ++e) tal_store(t.boxes, t.f32_out, ba * 4u + e, box[e]);
}

// -------------------------------------------------------------------------------------------------------------------- scores
// grid (G, B), 256 threads: a lane per element of the image's (A, nc) scores, every element written once
__global__ __launch_bounds__(kThreads) void k_tal_scores(const TalArgs t) {
    const int b = blockIdx.y;
    const uint32_t n = (uint32_t)t.A * (uint32_t)t.nc, step = gridDim.x * kThreads;   // A * nc < 2^31
    for (uint32_t e = blockIdx.x * kThreads + threadIdx.x; e < n; e += step) {
        const uint32_t a = e / (uint32_t)t.nc, c = e - a * (uint32_t)t.nc;
        const size_t ba = (size_t)b * t.A + a;
        const int g = t.row[ba];
        double v = 0.0;
        if (g >= 0 && (int64_t)c == t.labels[ba]) {
            const double pa = __longlong_as_double((long long)t.pos_al[(size_t)b * t.M + g]);
            const double po = __longlong_as_double((long long)t.pos_ov[(size_t)b * t.M + g]);
            v = __ddiv_rn(__dmul_rn(t.val[ba], po), __dadd_rn(pa, 1e-9));
        }
        tal_store(t.scores, t.f32_out, (size_t)b * n + e, v);
    }
}

}  // namespace evrep
