// evrep_detloss.hip -- the loss terms of ev-YOLOv6's ComputeLoss.__call__ (yolov6/models/losses/loss.py:176-217 with
// VarifocalLoss, BboxLoss and yolov6/utils/figure_iou.py's IOUloss(xyxy, giou, 1e-10)) and bbox_decode (loss.py:238-244) for the
// B images of a batch: values AND the gradients with respect to pred_scores and pred_distri in the forward launches, with no
// one-hot tensor, no compaction of the foreground rows and no host read.  include/evrep.h states the rules with evrep_detloss.
//
//   k_detloss_decode  a lane per (image, anchor, side): the side's expectation, its coordinate in stride units and in pixels.
//   k_detloss_rows    a lane per (image, anchor), chunks of 256 anchors dealt to at most kDetlossSlices workgroups round robin:
//                     w[b, a] = the row of target_scores added left to right; the workgroup's w added in a fixed order is its
//                     slice of tss.
//   k_detloss_cls     grid (G, B), a lane per element of the image's (A, nc) scores: the varifocal term and its gradient.  Every
//                     workgroup folds the tss slices itself (detloss_fold: the same additions in the same order everywhere) and
//                     leaves one partial sum.
//   k_detloss_box     grid (ceil(A / 256), B), four lanes per anchor, one per side: a foreground anchor decodes its box, forms the
//                     GIoU and DFL terms and writes its 4K gradients; the workgroup then zeroes the rows of its background
//                     anchors, a lane per element.  One partial of each of (iou, dfl, count) per workgroup.
//   k_detloss_fold    one workgroup: folds the partials in index order, divides by norm, writes losses[5].
//
// ROUNDING.  Every statement is ONE float64 operation written with __dadd_rn / __dsub_rn / __dmul_rn / __ddiv_rn; float32
// inputs are widened exactly; the one float32 quantity is aps = anc / stride.  exp and log are the double library functions.
// max(a, b) is a > b ? a : b, min(a, b) is a < b ? a : b.  The library is compiled with -ffp-contract=off and this file
// repeats it as a pragma.  Gradients are formed in float64 and rounded once at the store.
//
// Every loop ends at a value the host passed; every index is below the size the host stated (the DFL bin of a target is held
// to [0, R - 1] whatever the inputs).  Plain C++ stores, one integer atomicOr for the status word, no floating-point atomic,
// nothing read back, no allocation: the launches can be captured into a graph.
//
// evrep_detloss_distill (loss_distill.py) runs the rows, box and fold kernels as their <true> instances: the rows launch also
// leaves W (the w of the foreground anchors) and their count per slice, norm is tss > 0 ? tss : 1, and a foreground side adds
// its distillation term and gradient (evrep_kd.h).  The <false> instances are evrep_detloss, bit for bit what they were; the
// class launch of the distillation entry is k_detdistill_cls (evrep_detdistill.hip), which shares detloss_vfl.
#pragma once
#include "evrep_common.h"
#include "evrep_dfl.h"
#include "evrep_kd.h"

#pragma clang fp contract(off)

namespace evrep {

constexpr double kBceEps = (double)1e-12f;                               // torch's EPSILON of binary_cross_entropy_backward: a float
constexpr int kDetlossSlices = 256;                                    // slices of tss at most: one per lane of a folding workgroup

struct DetlossArgs {
    const float *p;               // (B, A, nc) pred_scores
    const float *z;               // (B, A, 4K) pred_distri, K = R + 1 with DFL, 1 without
    const float *anc;             // (A, 2)
    const float *stride;          // (A)
    const int64_t *labels;        // (B, A)
    const void *tb;               // (B, A, 4) double or float, pixels
    const void *ts;               // (B, A, nc) double or float
    const uint8_t *fg;            // (B, A)
    double *losses;               // [5]
    float *gs;                    // (B, A, nc) or null
    float *gz;                    // (B, A, 4K) or null
    float *boxes_s, *boxes_px;    // (B, A, 4): k_detloss_decode only
    uint32_t *status;             // (B)
    double *w;                    // scratch (B, A): the rows of target_scores
    double *tss_part;             // scratch [n_tss]
    double *cls_part;             // scratch [B * Gc]
    double *iou_part, *dfl_part, *cnt_part;   // scratch [B * Ga]
    double wc, wi, wd;
    uint32_t n_tss, n_cls, n_box;
    int32_t B, A, nc, R, K, use_dfl, f32_t, grad;
    // evrep_detloss_distill only
    const float *tp, *tz;         // the teacher's (B, A, nc) pred_scores and (B, A, 4K) pred_distri
    double *wfg_part, *nfg_part;  // scratch [n_tss]: the w and the count of the foreground anchors per slice
    double *dcls_part;            // scratch [n_cls]
    double *ddfl_part;            // scratch [n_box]
    double T, k_class, k_dfl;     // temperature, decay * distill_weight["class"], decay * distill_weight["dfl"]
};

// loss.py divides by tss where it exceeds 1, loss_distill.py where it exceeds 0 (:225, :426, :449; target scores are >= 0)
template <bool D>
__device__ inline double detloss_norm(double tss) {
    return D ? (tss > 0.0 ? tss : 1.0) : (tss > 1.0 ? tss : 1.0);
}

__device__ inline double dl_target(const void *base, size_t at, int f32_t) {
    return f32_t ? (double)static_cast<const float *>(base)[at] : static_cast<const double *>(base)[at];
}

// the sum over a workgroup of 256 in a fixed order: lanes by a butterfly (every lane ends with the same bits), the waves in
// ascending order.  Valid in every thread.  Contains __syncthreads().
__device__ inline double detloss_block_sum(double s, double *tmp) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s = __dadd_rn(s, __shfl_xor(s, d, 64));
    if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = s;
    __syncthreads();
    double r = tmp[0];
#pragma unroll
    for (int wv = 1; wv < kWaves; ++wv) r = __dadd_rn(r, tmp[wv]);
    __syncthreads();
    return r;
}

// n partials in a fixed order: thread t adds t, t + 256, ... ascending, then the workgroup's sum
__device__ inline double detloss_fold(const double *__restrict__ part, uint32_t n, double *tmp) {
    double s = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) s = __dadd_rn(s, part[i]);
    return detloss_block_sum(s, tmp);
}

// one side e of anchor a: the centre's coordinate in stride units (float32, widened), the side's expectation (the distance itself
// without DFL) and the box's coordinate; z: the side's K values
__device__ inline void detloss_coord(const DetlossArgs &t, const float *__restrict__ z, int a, int e, double &c, double &m, double &Z,
                                     double &d, double &v) {
    c = (double)__fdiv_rn(t.anc[(size_t)a * 2u + (size_t)(e & 1)], t.stride[a]);
    if (t.use_dfl) {
        dfl_side(z, 1, t.K, m, Z, d);                                    // evrep_dfl.h: one side of bbox_decode
    } else {
        m = 0.0; Z = 1.0; d = (double)z[0];
    }
    v = e < 2 ? __dsub_rn(c, d) : __dadd_rn(c, d);
}

// -------------------------------------------------------------------------------------------------------------------- decode
// grid (ceil(4 A / 256), B), 256 threads: a lane per (anchor, side), the K logits of neighbouring lanes adjoin in memory
__global__ __launch_bounds__(kThreads) void k_detloss_decode(const DetlossArgs t) {
    const int b = blockIdx.y;
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;              // 4 A <= 2^26
    if (i >= 4u * (uint32_t)t.A) return;
    const int a = (int)(i >> 2), e = (int)(i & 3u);
    const size_t at = ((size_t)b * t.A + a) * 4u + e;
    double c, m, Z, d, v;
    detloss_coord(t, t.z + at * (size_t)t.K, a, e, c, m, Z, d, v);
    t.boxes_s[at] = (float)v;
    t.boxes_px[at] = (float)__dmul_rn(v, (double)t.stride[a]);
}

// ---------------------------------------------------------------------------------------------------------------------- rows
// grid (n_tss), 256 threads: chunk c of 256 (image, anchor) pairs belongs to slice c % n_tss
template <bool D>
__global__ __launch_bounds__(kThreads) void k_detloss_rows(const DetlossArgs t) {
    __shared__ double tmp[kWaves];
    const size_t n = (size_t)t.B * (size_t)t.A, step = (size_t)gridDim.x * kThreads;
    double s = 0.0, sw = 0.0, sn = 0.0;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += step) {
        const size_t at = i * (size_t)t.nc;
        double w = 0.0;
        for (int c = 0; c < t.nc; ++c) w = __dadd_rn(w, dl_target(t.ts, at + c, t.f32_t));
        t.w[i] = w;
        s = __dadd_rn(s, w);
        if (D && t.fg[i] != 0) {
            sw = __dadd_rn(sw, w);
            sn = __dadd_rn(sn, 1.0);
        }
    }
    const double tot = detloss_block_sum(s, tmp);
    if (threadIdx.x == 0) t.tss_part[blockIdx.x] = tot;
    if (D) {                                                           // before the box launch: every foreground gradient needs both
        const double tw = detloss_block_sum(sw, tmp), tn = detloss_block_sum(sn, tmp);
        if (threadIdx.x == 0) {
            t.wfg_part[blockIdx.x] = tw;
            t.nfg_part[blockIdx.x] = tn;
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- class term
// one element of VarifocalLoss: the term bce * wt and, with grad, d term / d p
__device__ inline void detloss_vfl(double p, double q, bool lab, bool grad, double &term, double &g) {
    const double wt = lab ? q : __dmul_rn(__dmul_rn(0.75, p), p);
    const double omp = __dsub_rn(1.0, p);
    const double lp = dl_max(log(p), -100.0), lq = dl_max(log(omp), -100.0);
    const double bce = -__dadd_rn(__dmul_rn(q, lp), __dmul_rn(__dsub_rn(1.0, q), lq));
    term = __dmul_rn(bce, wt);
    g = 0.0;
    if (grad) {
        const double db = __ddiv_rn(__dsub_rn(p, q), dl_max(__dmul_rn(omp, p), kBceEps));
        g = __dmul_rn(db, wt);
        if (!lab) g = __dadd_rn(g, __dmul_rn(bce, __dmul_rn(1.5, p)));
    }
}

// grid (Gc, B), 256 threads: a lane per element of the image's (A, nc) scores
__global__ __launch_bounds__(kThreads) void k_detloss_cls(const DetlossArgs t) {
    __shared__ double tmp[kWaves];
    const int b = blockIdx.y;
    const double tss = detloss_fold(t.tss_part, t.n_tss, tmp);
    const double norm = tss > 1.0 ? tss : 1.0;
    const double sc = __ddiv_rn(t.wc, norm);
    const uint32_t n = (uint32_t)t.A * (uint32_t)t.nc, step = gridDim.x * kThreads;   // A * nc < 2^31
    double s = 0.0;
    for (uint32_t e = blockIdx.x * kThreads + threadIdx.x; e < n; e += step) {
        const uint32_t a = e / (uint32_t)t.nc, c = e - a * (uint32_t)t.nc;
        const size_t ba = (size_t)b * t.A + a, at = (size_t)b * n + e;
        const double p = (double)t.p[at], q = dl_target(t.ts, at, t.f32_t);
        const bool lab = t.fg[ba] != 0 && t.labels[ba] == (int64_t)c;
        double term, g;
        detloss_vfl(p, q, lab, t.grad != 0, term, g);
        s = __dadd_rn(s, term);
        if (t.grad) t.gs[at] = (float)__dmul_rn(sc, g);
    }
    const double tot = detloss_block_sum(s, tmp);
    if (threadIdx.x == 0) t.cls_part[(size_t)b * gridDim.x + blockIdx.x] = tot;
}

// ------------------------------------------------------------------------------------------------------------------ box terms
// the gradient a min / max hands to its first argument: all of it where it is the one taken, half at a tie
__device__ inline double dl_take(bool first, bool tie, double g) { return tie ? __dmul_rn(0.5, g) : (first ? g : 0.0); }

__device__ inline double dl_quad(double v, int lane) { return __shfl(v, lane, 64); }

// grid (Ga, B), 256 threads; status[b] was zeroed by a memset ordered before this launch.  A workgroup owns 256 consecutive
// anchors and walks them in four rounds of 64, FOUR LANES PER ANCHOR, one per side: the K logits of neighbouring lanes adjoin in
// memory and a foreground anchor's chain of exponentials is a quarter as long.  The four lanes exchange their coordinates and
// side terms by shuffles that every lane executes, then each forms the anchor's GIoU terms itself (the same bits in all four).
// <true>: a foreground side also forms the softmaxes of its own and the teacher's K logits at temperature T, its row of the
// distillation sum, and adds cdd * (ps_k * sum(pt) - pt_k) to its gradients before the one store.
template <bool D>
__global__ __launch_bounds__(kThreads) void k_detloss_box(const DetlossArgs t) {
    __shared__ double tmp[kWaves];
    __shared__ uint8_t s_fg[kThreads];
    const int b = blockIdx.y, tid = threadIdx.x, e = tid & 3, a0 = blockIdx.x * kThreads, A = t.A, K = t.K;
    const int quad = (tid & 63) & ~3;                                   // the wave's lane of the anchor's side 0
    const double tss = detloss_fold(t.tss_part, t.n_tss, tmp);
    const double norm = detloss_norm<D>(tss);
    const double eps = 1e-10;
    double l_iou = 0.0, l_dfl = 0.0, n_fg = 0.0, l_dd = 0.0, cdd = 0.0;
    if (D && t.use_dfl && t.grad) {                                    // the same additions in the same order in every workgroup
        const double W = detloss_fold(t.wfg_part, t.n_tss, tmp), nf = detloss_fold(t.nfg_part, t.n_tss, tmp);
        if (nf > 0.0)
            cdd = __ddiv_rn(__ddiv_rn(__dmul_rn(__dmul_rn(__dmul_rn(t.wd, t.k_dfl), t.T), W), norm), __dmul_rn(4.0, nf));
    }
    for (int round = 0; round < 4; ++round) {
        const int slot = round * 64 + (tid >> 2), a = a0 + slot;
        const bool in = a < A;
        const size_t ba = (size_t)b * A + (in ? a : 0);
        const bool fg = in && t.fg[ba] != 0;                           // (the same in the anchor's four lanes)
        if (e == 0) s_fg[slot] = fg ? 1 : 0;
        const float *z = t.z + (ba * 4u + e) * (size_t)K;
        double c = 0.0, m = 0.0, Z = 1.0, d = 0.0, v = 0.0, tv = 0.0, side = 0.0, wl = 0.0, wr = 0.0;
        double ms = 0.0, Zs = 1.0, mt = 0.0, Zt = 1.0, spt = 0.0;
        const float *tz = D ? t.tz + (ba * 4u + e) * (size_t)K : nullptr;
        int tl = 0;
        if (fg) {
            detloss_coord(t, z, a, e, c, m, Z, d, v);
            tv = __ddiv_rn(dl_target(t.tb, ba * 4u + e, t.f32_t), (double)t.stride[a]);
            if (t.use_dfl) {
                const double dist = e < 2 ? __dsub_rn(c, tv) : __dsub_rn(tv, c);
                const double u = dl_min(dl_max(dist, 0.0), __dsub_rn((double)t.R, 0.01));
                tl = (u >= 0.0 && u < (double)t.R) ? (int)u : 0;          // (a NaN: bin 0; the index stays inside the K logits)
                if (tl > t.R - 1) tl = t.R - 1;
                wl = __dsub_rn((double)(tl + 1), u);
                wr = __dsub_rn(1.0, wl);
                const double lse = __dadd_rn(m, log(Z));
                const double cl = __dsub_rn(lse, (double)z[tl]), cr = __dsub_rn(lse, (double)z[tl + 1]);
                side = __dadd_rn(__dmul_rn(cl, wl), __dmul_rn(cr, wr));
                if (D) {
                    double kl;
                    kd_stats(z, K, t.T, ms, Zs);
                    kd_stats(tz, K, t.T, mt, Zt);
                    kd_row(z, tz, K, t.T, ms, Zs, mt, Zt, kl, spt);
                    l_dd = __dadd_rn(l_dd, kl);
                }
            }
        }
        // every lane takes part: a quad's values come from its own four lanes
        const double x1 = dl_quad(v, quad), y1 = dl_quad(v, quad + 1), x2 = dl_quad(v, quad + 2), y2 = dl_quad(v, quad + 3);
        const double tx1 = dl_quad(tv, quad), ty1 = dl_quad(tv, quad + 1), tx2 = dl_quad(tv, quad + 2), ty2 = dl_quad(tv, quad + 3);
        const double sd0 = dl_quad(side, quad), sd1 = dl_quad(side, quad + 1), sd2 = dl_quad(side, quad + 2), sd3 = dl_quad(side, quad + 3);
        if (fg) {
            const double w = t.w[ba];
            if (e == 0) {
                const int64_t lab = t.labels[ba];
                if (lab < 0 || lab >= (int64_t)t.nc) atomicOr(&t.status[b], EVREP_DETLOSS_ST_BAD_LABEL);
            }
            // IOUloss, giou
            const double iwr = __dsub_rn(dl_min(x2, tx2), dl_max(x1, tx1)), ihr = __dsub_rn(dl_min(y2, ty2), dl_max(y1, ty1));
            const double iw = dl_max(iwr, 0.0), ih = dl_max(ihr, 0.0);
            const double inter = __dmul_rn(iw, ih);
            const double w1 = __dsub_rn(x2, x1), h1 = __dadd_rn(__dsub_rn(y2, y1), eps);
            const double w2 = __dsub_rn(tx2, tx1), h2 = __dadd_rn(__dsub_rn(ty2, ty1), eps);
            const double uni = __dadd_rn(__dsub_rn(__dadd_rn(__dmul_rn(w1, h1), __dmul_rn(w2, h2)), inter), eps);
            const double iou = __ddiv_rn(inter, uni);
            const double cw = __dsub_rn(dl_max(x2, tx2), dl_min(x1, tx1)), ch = __dsub_rn(dl_max(y2, ty2), dl_min(y1, ty1));
            const double ca = __dadd_rn(__dmul_rn(cw, ch), eps);
            const double num = __dsub_rn(ca, uni);
            const double giou = __dsub_rn(iou, __ddiv_rn(num, ca));
            if (e == 0) {
                l_iou = __dadd_rn(l_iou, __dmul_rn(__dsub_rn(1.0, giou), w));
                if (t.use_dfl) {
                    const double dfl = __ddiv_rn(__dadd_rn(__dadd_rn(__dadd_rn(sd0, sd1), sd2), sd3), 4.0);
                    l_dfl = __dadd_rn(l_dfl, __dmul_rn(dfl, w));
                }
                n_fg = __dadd_rn(n_fg, 1.0);
            }
            if (t.grad) {
                // backwards through IOUloss, statement by statement: g is dL / d(1 - giou)
                const double g = __ddiv_rn(__dmul_rn(t.wi, w), norm);
                const double g_num = __ddiv_rn(g, ca);
                const double g_ca = __dsub_rn(g_num, __ddiv_rn(__dmul_rn(g, num), __dmul_rn(ca, ca)));
                const double g_iou = -g;
                const double g_uni = __dsub_rn(-g_num, __ddiv_rn(__dmul_rn(g_iou, inter), __dmul_rn(uni, uni)));
                const double g_int = __dsub_rn(__ddiv_rn(g_iou, uni), g_uni);
                const double g_w1 = __dmul_rn(g_uni, h1), g_h1 = __dmul_rn(g_uni, w1);
                const double g_iw = iwr >= 0.0 ? __dmul_rn(g_int, ih) : 0.0, g_ih = ihr >= 0.0 ? __dmul_rn(g_int, iw) : 0.0;
                const double g_cw = __dmul_rn(g_ca, ch), g_ch = __dmul_rn(g_ca, cw);
                // x1: -max(x1, tx1) of iw, -min(x1, tx1) of cw, -w1; x2: +min(x2, tx2) of iw, +max(x2, tx2) of cw, +w1;
                // x1 = ax - d_l, x2 = ax + d_r: the side's distance takes -g_x1 or +g_x2
                double g_d;
                if (e == 0) g_d = -__dsub_rn(__dsub_rn(-dl_take(x1 > tx1, x1 == tx1, g_iw), dl_take(x1 < tx1, x1 == tx1, g_cw)), g_w1);
                else if (e == 1) g_d = -__dsub_rn(__dsub_rn(-dl_take(y1 > ty1, y1 == ty1, g_ih), dl_take(y1 < ty1, y1 == ty1, g_ch)), g_h1);
                else if (e == 2) g_d = __dadd_rn(__dadd_rn(dl_take(x2 < tx2, x2 == tx2, g_iw), dl_take(x2 > tx2, x2 == tx2, g_cw)), g_w1);
                else g_d = __dadd_rn(__dadd_rn(dl_take(y2 < ty2, y2 == ty2, g_ih), dl_take(y2 > ty2, y2 == ty2, g_ch)), g_h1);
                float *gz = t.gz + (ba * 4u + e) * (size_t)K;
                if (t.use_dfl) {
                    const double cd = __ddiv_rn(__ddiv_rn(__dmul_rn(t.wd, w), norm), 4.0);
                    for (int k = 0; k < K; ++k) {
                        const double pr = __ddiv_rn(exp(__dsub_rn((double)z[k], m)), Z);
                        const double v1 = __dmul_rn(g_d, __dmul_rn(pr, __dsub_rn((double)k, d)));
                        double v2 = pr;
                        if (k == tl) v2 = __dsub_rn(v2, wl);
                        if (k == tl + 1) v2 = __dsub_rn(v2, wr);
                        double gk = __dadd_rn(v1, __dmul_rn(cd, v2));
                        if (D) {
                            const double ps = kd_prob(z[k], t.T, ms, Zs), pt = kd_prob(tz[k], t.T, mt, Zt);
                            gk = __dadd_rn(gk, __dmul_rn(cdd, __dsub_rn(__dmul_rn(ps, spt), pt)));
                        }
                        gz[k] = (float)gk;
                    }
                } else {
                    gz[0] = (float)g_d;
                }
            }
        }
    }
    __syncthreads();
    if (t.grad) {                                                      // the rows of the background anchors, a lane per element
        const int na = A - a0 < kThreads ? A - a0 : kThreads;
        const uint32_t per = 4u * (uint32_t)K, ne = (uint32_t)na * per;
        float *gz0 = t.gz + ((size_t)b * A + a0) * per;
        for (uint32_t i = tid; i < ne; i += kThreads)
            if (!s_fg[i / per]) gz0[i] = 0.0f;
    }
    const double s_iou = detloss_block_sum(l_iou, tmp), s_dfl = detloss_block_sum(l_dfl, tmp);
    const double s_cnt = detloss_block_sum(n_fg, tmp);
    if (tid == 0) {
        const size_t at = (size_t)b * gridDim.x + blockIdx.x;
        t.iou_part[at] = s_iou;
        t.dfl_part[at] = s_dfl;
        t.cnt_part[at] = s_cnt;
    }
    if (D) {
        const double s_dd = detloss_block_sum(l_dd, tmp);
        if (tid == 0) t.ddfl_part[(size_t)b * gridDim.x + blockIdx.x] = s_dd;
    }
}

// ---------------------------------------------------------------------------------------------------------------------- fold
// one workgroup of 256.  <true>: losses[8] = loss_cls, loss_iou, loss_dfl, d_loss_cls, d_loss_dfl, tss, n_fg, W
template <bool D>
__global__ __launch_bounds__(kThreads) void k_detloss_fold(const DetlossArgs t) {
    __shared__ double tmp[kWaves];
    const double tss = detloss_fold(t.tss_part, t.n_tss, tmp);
    const double cls = detloss_fold(t.cls_part, t.n_cls, tmp);
    const double iou = detloss_fold(t.iou_part, t.n_box, tmp), dfl = detloss_fold(t.dfl_part, t.n_box, tmp);
    const double cnt = detloss_fold(t.cnt_part, t.n_box, tmp);
    double dcls = 0.0, ddfl = 0.0, W = 0.0;
    if (D) {
        dcls = detloss_fold(t.dcls_part, t.n_cls, tmp);
        ddfl = detloss_fold(t.ddfl_part, t.n_box, tmp);
        W = detloss_fold(t.wfg_part, t.n_tss, tmp);
    }
    if (threadIdx.x == 0) {
        const double norm = detloss_norm<D>(tss);
        t.losses[0] = __ddiv_rn(cls, norm);
        t.losses[1] = __ddiv_rn(iou, norm);
        t.losses[2] = __ddiv_rn(dfl, norm);
        if (D) {
            const double T2 = __dmul_rn(t.T, t.T);
            t.losses[3] = __dmul_rn(T2, dcls);
            // the reference's mean over the 4 * n_fg rows, times T^2, times every foreground anchor's w, over norm
            t.losses[4] = cnt > 0.0 ? __ddiv_rn(__dmul_rn(__dmul_rn(T2, __ddiv_rn(ddfl, __dmul_rn(4.0, cnt))), W), norm) : 0.0;
            t.losses[5] = tss;
            t.losses[6] = cnt;
            t.losses[7] = W;
        } else {
            t.losses[3] = tss;
            t.losses[4] = cnt;
        }
    }
}

}  // namespace evrep
