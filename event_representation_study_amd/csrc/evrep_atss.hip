// evrep_atss.hip -- the training targets of the warm-up epochs: ATSSAssigner.forward (ev-YOLOv6 yolov6/assigners/atss_assigner.py
// with iou2d_calculator.py and assigner_utils.py behind it), what ComputeLoss.__call__ assigns with while epoch_num < warmup_epoch
// (yolov6/models/losses/loss.py:84-97), for the B images of a batch with no (B, M, A) array in memory.  include/evrep.h states
// the rules with evrep_atss_assign.  The rows, the in-box test, the IoU against the predicted box and the finite check are those
// of evrep_assign.hip.
//
//   k_atss_prepare   grid (G, B): every value of the image's labels and predicted boxes is looked at once; a non-finite one sets
//                    EVREP_TAL_ST_NONFINITE in status[b].  Clears the per-anchor words of the scratch.
//   k_atss_select    one workgroup per (image, row).  Per level a valid row streams the level's anchors in chunks of 256, a lane
//                    per anchor (beginning at the chunk of the nearest anchor and going outwards), and keeps the first `topk` of the total order (centre distance ascending, anchor ascending) in
//                    LDS (the TopkList of evrep_assign.hip, under this order); the key is the distance's bits (non-negative doubles order
//                    as their bits).  The n_levels * topk <= 256 candidates then have a lane each: the lane computes the
//                    candidate's IoU with the anchor box, every lane adds the values in the fixed order (level, place) to the
//                    mean and the deviation, and a candidate above the threshold whose centre lies in the box adds 1 to
//                    cnt[b, a] and takes min(first[b, a], m): integer atomics, free of order.
//   k_atss_resolve   a lane per (image, anchor): c = cnt; the row is first (c == 1) or the first row of greatest anchor IoU over
//                    all M rows (c > 1); writes the label, the box, fg, and keeps the row and the score value in the scratch.
//   k_atss_scores    a lane per element of target_scores: zero, or the kept value at a foreground anchor's label.
//
// ROUNDING as in evrep_assign.hip: every statement is one operation of the type evrep.h states, written with the __d*_rn /
// __f*_rn intrinsics; max(a, b) is a > b ? a : b and min(a, b) is a < b ? a : b.
//
// Every loop ends at a value the host passed; every index is below the size the host stated.  Plain C++ stores, integer
// atomics only, nothing read back, no allocation: the launches can be captured into a graph.
#pragma once
#include "evrep_assign.hip"

#pragma clang fp contract(off)

namespace evrep {

constexpr int kAtssMaxTopk = EVREP_ATSS_MAX_TOPK;
constexpr int kAtssMaxLevels = EVREP_ATSS_MAX_LEVELS;
constexpr int kAtssThreads = 256;                                      // k_atss_select: a chunk of anchors, or the candidates, a lane each
static_assert(EVREP_ATSS_MAX_CANDIDATES == kAtssThreads, "a candidate has a lane");

struct AtssArgs {
    const float *anchors;         // (A, 4) xyxy
    const float *pd_bboxes;       // (B, A, 4) or null
    const double *gt;             // (B, M, 5)
    int64_t *labels;              // (B, A)
    void *boxes;                  // (B, A, 4) double or float
    void *scores;                 // (B, A, nc) double or float
    uint8_t *fg;                  // (B, A)
    uint32_t *status;             // (B)
    uint32_t *cnt;                // scratch (B, A): the rows an anchor is a positive of
    uint32_t *first;              // scratch (B, A): the lowest of them
    int32_t *row;                 // scratch (B, A): the assigned row, -1 for background
    double *val;                  // scratch (B, A): the value at the label's place in target_scores
    int32_t lvl_start[kAtssMaxLevels], lvl_n[kAtssMaxLevels];
    int32_t B, M, A, nc, topk, n_levels, f32_boxes, f32_scores;
};

struct AtssAnchor {
    double x1, y1, x2, y2, area, cx, cy;
};

// the float32 quantities of an anchor box, widened: its area and its centre
__device__ inline AtssAnchor atss_anchor(const float *anchors, int a) {
    const float *p = anchors + (size_t)a * 4u;                         // a < A
    const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
    AtssAnchor n;
    n.x1 = (double)x1; n.y1 = (double)y1; n.x2 = (double)x2; n.y2 = (double)y2;
    n.area = (double)__fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1));
    n.cx = (double)__fdiv_rn(__fadd_rn(x1, x2), 2.0f);
    n.cy = (double)__fdiv_rn(__fadd_rn(y1, y2), 2.0f);
    return n;
}

// bbox_overlaps(row, anchor box), mode iou
__device__ inline double atss_overlap(const TalRow &r, const AtssAnchor &n) {
    const double w = tal_max(__dsub_rn(tal_min(r.x2, n.x2), tal_max(r.x1, n.x1)), 0.0);
    const double h = tal_max(__dsub_rn(tal_min(r.y2, n.y2), tal_max(r.y1, n.y1)), 0.0);
    const double ov = __dmul_rn(w, h);
    const double area_g = __dmul_rn(__dsub_rn(r.x2, r.x1), __dsub_rn(r.y2, r.y1));
    const double u = tal_max(__dsub_rn(__dadd_rn(area_g, n.area), ov), 1e-6);
    return __ddiv_rn(ov, u);
}

// the distance of the centres
__device__ inline double atss_distance(const TalRow &r, const AtssAnchor &n) {
    const double dx = __dsub_rn(__ddiv_rn(__dadd_rn(r.x1, r.x2), 2.0), n.cx);
    const double dy = __dsub_rn(__ddiv_rn(__dadd_rn(r.y1, r.y2), 2.0), n.cy);
    return __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
}

// ------------------------------------------------------------------------------------------------------------------- prepare
// grid (G, B), 256 threads; status[b] was zeroed by a memset ordered before this launch
__global__ __launch_bounds__(kThreads) void k_atss_prepare(const AtssArgs t) {
    const int b = blockIdx.y;
    const size_t start = (size_t)blockIdx.x * kThreads + threadIdx.x, step = (size_t)gridDim.x * kThreads;
    const size_t n_b = (size_t)t.A * 4u, n_g = (size_t)t.M * 5u;
    bool bad = t.pd_bboxes && any_nonfinite(t.pd_bboxes + (size_t)b * n_b, n_b, start, step);
    bad = bad || any_nonfinite(t.gt + (size_t)b * n_g, n_g, start, step);
    claims_clear(t.cnt, t.first, b, t.A, start, step);
    raise_nonfinite(bad, &t.status[b]);
}

// -------------------------------------------------------------------------------------------------------------------- select
// an entry of the order: the distance's bits and the anchor
struct AtssBefore {
    __device__ bool operator()(unsigned long long k1, uint32_t i1, unsigned long long k2, uint32_t i2) const {
        return k1 < k2 || (k1 == k2 && i1 < i2);
    }
};
using AtssList = TopkList<kAtssMaxTopk, kAtssThreads, AtssBefore>;

// the first entry of the order among a wave's lanes, in every lane
__device__ inline void atss_wave_first(unsigned long long &k, uint32_t &i) {
    const AtssBefore before;
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)k, d, 64), hi = __shfl_xor((uint32_t)(k >> 32), d, 64), oi = __shfl_xor(i, d, 64);
        const unsigned long long ok = ((unsigned long long)hi << 32) | lo;
        if (before(ok, oi, k, i)) {
            k = ok;
            i = oi;
        }
    }
}

// grid (M, B), 256 threads; every level holds at least topk anchors and n_levels * topk <= 256 (held by the host)
__global__ __launch_bounds__(kAtssThreads) void k_atss_select(const AtssArgs t) {
    __shared__ AtssList::Storage s_list;
    __shared__ unsigned long long s_wk[kAtssThreads / 64];             // a level's nearest anchor: the waves' entries
    __shared__ uint32_t s_wi[kAtssThreads / 64];
    __shared__ uint32_t s_cand[kAtssThreads];
    __shared__ double s_v[kAtssThreads];
    const AtssBefore before;
    const int tid = threadIdx.x, m = blockIdx.x, b = blockIdx.y, A = t.A, K = t.topk;
    if (t.status[b] & EVREP_TAL_ST_NONFINITE) return;                   // (uniform: written by the launch before this one)
    const TalRow r = tal_row(t.gt, b, t.M, m);
    if (!tal_row_valid(r)) return;
    if (tal_class(r.cls, t.nc) < 0) {
        if (tid == 0) atomicOr(&t.status[b], EVREP_TAL_ST_BAD_CLASS);
        return;
    }
    for (int l = 0; l < t.n_levels; ++l) {
        const int s0 = t.lvl_start[l], n_l = t.lvl_n[l];                // s0 + n_l <= A, n_l >= K
        // The list is the first K of a total order: the order of the walk does not change it, only how many chunks displace
        // entries and pay the merge.  A level is stored row by row, so a walk from its first chunk comes nearer with every
        // chunk; this one begins at the chunk that holds the level's nearest anchor and goes outwards on both sides.
        unsigned long long bk = ~0ull;
        uint32_t bi = 0xFFFFFFFFu;
        for (int j = tid; j < n_l; j += kAtssThreads) {
            const uint32_t ia = (uint32_t)(s0 + j);                     // < A
            const unsigned long long kb = (unsigned long long)__double_as_longlong(atss_distance(r, atss_anchor(t.anchors, (int)ia)));
            if (before(kb, ia, bk, bi)) {
                bk = kb;
                bi = ia;
            }
        }
        atss_wave_first(bk, bi);
        if ((tid & 63) == 0) {
            s_wk[tid >> 6] = bk;
            s_wi[tid >> 6] = bi;
        }
        __syncthreads();
        for (int w = 0; w < kAtssThreads / 64; ++w) {
            if (before(s_wk[w], s_wi[w], bk, bi)) {
                bk = s_wk[w];
                bi = s_wi[w];
            }
        }
        __syncthreads();
        const int n_ch = (n_l + kAtssThreads - 1) / kAtssThreads, c0 = ((int)bi - s0) / kAtssThreads;   // s0 <= bi < s0 + n_l: n_l >= 1
        AtssList list(s_list, K);
        for (int i = 0; i < 2 * n_ch - 1; ++i) {                       // c0, c0 + 1, c0 - 1, c0 + 2, ...: every chunk once
            const int dd = (i + 1) >> 1, c = (i & 1) ? c0 + dd : c0 - dd;
            if (c < 0 || c >= n_ch) continue;                          // (uniform)
            const int j = c * kAtssThreads + tid;
            const bool in = j < n_l;
            const uint32_t ia = (uint32_t)(s0 + (in ? j : 0));          // < A
            list.offer(in, (unsigned long long)__double_as_longlong(atss_distance(r, atss_anchor(t.anchors, (int)ia))), ia);
        }
        if (tid < K) s_cand[l * K + tid] = list.index(tid);             // size() == K: the level holds at least K anchors; l * K + tid < 256
        __syncthreads();
    }
    const int n = t.n_levels * K;                                      // <= 256
    AtssAnchor an;
    double o = 0.0;
    if (tid < n) {
        an = atss_anchor(t.anchors, (int)s_cand[tid]);
        o = atss_overlap(r, an);
        s_v[tid] = o;
    }
    __syncthreads();
    // every lane walks the candidates in the order (level, place): the same sums in every lane
    // (0 + v_0 is v_0: the values are never -0)
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum = __dadd_rn(sum, s_v[i]);
    const double mean = __ddiv_rn(sum, (double)n);
    double ss = 0.0;
    for (int i = 0; i < n; ++i) {
        const double dv = __dsub_rn(s_v[i], mean);
        ss = __dadd_rn(ss, __dmul_rn(dv, dv));
    }
    const double thr = __dadd_rn(mean, __dsqrt_rn(__ddiv_rn(ss, (double)(n - 1))));   // n == 1: 0 / 0, no positives
    if (tid < n && o > thr && tal_in_gt(r, an.cx, an.cy)) {
        const int a = (int)s_cand[tid];                                // < A
        atomicAdd(&t.cnt[(size_t)b * A + a], 1u);
        atomicMin(&t.first[(size_t)b * A + a], (uint32_t)m);
    }
}

// ------------------------------------------------------------------------------------------------------------------- resolve
// grid (ceil(A / 256), B), 256 threads.  M == 0: the reference's early return
__global__ __launch_bounds__(kThreads) void k_atss_resolve(const AtssArgs t) {
    const int b = blockIdx.y, a = blockIdx.x * kThreads + threadIdx.x, A = t.A, M = t.M;
    if (a >= A) return;
    const size_t ba = (size_t)b * A + a;
    uint32_t c = 0u;
    int g = 0;
    double box[4] = {0.0, 0.0, 0.0, 0.0}, v = 0.0;
    int64_t label = (int64_t)t.nc;
    if (M > 0) {
        c = t.cnt[ba];
        if (c == 1u) {
            g = (int)t.first[ba];                                      // a row that claimed the anchor: < M
        } else if (c > 1u) {
            const AtssAnchor an = atss_anchor(t.anchors, a);
            double best = atss_overlap(tal_row(t.gt, b, M, 0), an);
            for (int m = 1; m < M; ++m) {
                const double w = atss_overlap(tal_row(t.gt, b, M, m), an);
                if (w > best) {
                    best = w;
                    g = m;
                }
            }
        }
        const TalRow r = tal_row(t.gt, b, M, g);
        box[0] = r.x1; box[1] = r.y1; box[2] = r.x2; box[3] = r.y2;
        if (c != 0u) {
            const int cl = tal_class(r.cls, t.nc);
            label = (int64_t)(cl < 0 ? 0 : cl);
            v = t.pd_bboxes ? (double)(float)tal_iou(r, tal_pbox(t.pd_bboxes, b, A, a)) : 1.0;
        }
    }
    t.labels[ba] = label;
    t.fg[ba] = c != 0u ? 1 : 0;
    t.row[ba] = c != 0u ? g : -1;
    t.val[ba] = v;
    for (int e = 0; e < 4; ++e) tal_store(t.boxes, t.f32_boxes, ba * 4u + e, box[e]);
}

// -------------------------------------------------------------------------------------------------------------------- scores
// grid (G, B), 256 threads: a lane per element of the image's (A, nc) scores, every element written once
__global__ __launch_bounds__(kThreads) void k_atss_scores(const AtssArgs t) {
    const int b = blockIdx.y;
    const uint32_t n = (uint32_t)t.A * (uint32_t)t.nc, step = gridDim.x * kThreads;   // A * nc < 2^31
    for (uint32_t e = blockIdx.x * kThreads + threadIdx.x; e < n; e += step) {
        const uint32_t a = e / (uint32_t)t.nc, c = e - a * (uint32_t)t.nc;
        const size_t ba = (size_t)b * t.A + a;
        const double v = (t.row[ba] >= 0 && (int64_t)c == t.labels[ba]) ? t.val[ba] : 0.0;
        tal_store(t.scores, t.f32_scores, (size_t)b * n + e, v);
    }
}

}  // namespace evrep
