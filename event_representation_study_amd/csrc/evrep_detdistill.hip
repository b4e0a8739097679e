// evrep_detdistill.hip -- the distillation losses of ev-YOLOv6's loss_distill.py (ComputeLoss.__call__ :62-279 with
// distill_loss_cls :281-292, BboxLoss.distill_loss_dfl :489-500 and distill_loss_cw :294-340): values AND the gradients with
// respect to the student's tensors, made by the forward launches.  include/evrep.h states the rules with
// evrep_detloss_distill and evrep_detloss_cwd.
//
// evrep_detloss_distill is FOUR launches behind the memset of status:
//   k_detloss_rows<true>   evrep_detloss.hip: w[b, a], the slices of tss, and per slice W (the w of the foreground anchors) and
//                          their count -- both enter every foreground gradient, so they exist before the box launch writes.
//   k_detdistill_cls       grid (Gd, B): a workgroup holds a tile of whole rows of p and of the teacher's tp in LDS (each is
//                          read from memory once) and alternates between a lane per ELEMENT for what is costly (x / T, exp,
//                          the quotients, the logarithms of the KL term, the varifocal term of detloss_vfl, shared with
//                          evrep_detloss) and a lane per ROW for what must run left to right and is cheap (the maximum, Z,
//                          sum(pt): comparisons and additions).  The element's gradient is written once: varifocal part plus
//                          distillation part, added in float64.
//   k_detloss_box<true>    evrep_detloss.hip: the box terms, a foreground side's distillation row and its gradients.
//   k_detloss_fold<true>   evrep_detloss.hip: losses[8].
//
// evrep_detloss_cwd is TWO launches:
//   k_detdistill_cw        a workgroup per (level, n, c) row of H * W floats of s and of t: four passes (maxima; sums of
//                          exponentials; the row's KL sum and sum(exp(lt)); the gradients, written once).  A row of at most
//                          kCwStage floats is staged in LDS in the first pass and the later passes read LDS; a longer row is
//                          re-read from memory (at 80 x 80 both rows are 51 KB, which stay in L2 between the passes).  A thread
//                          reads in every pass the elements it read in the first, so no barrier lies between a store to LDS and
//                          its load.  The maps' element types (EVREP_DT_*, the student's and the teacher's apart) are
//                          two codes, the same in every thread: a 16-bit element is widened exactly at the load (rule
//                          W1, evrep_f16.h) by a switch on the code -- the kernel is bound by its float64 arithmetic, so
//                          the switch replaces nine template instances; a second instance without the switch serves two
//                          float32 sides, which keep their time.  The LDS stage and the gradients stay float32.
//   k_detdistill_cw_fold   one workgroup: a level's partials in index order, times tau^2 / (N * C).
//
// ROUNDING as in evrep_detloss.hip: every statement is ONE float64 operation, float32 inputs widened exactly, x / T a float64
// division, exp and log the double library functions.  No floating-point atomic, plain C++ stores, every loop ends at a value
// the host passed, nothing read back, no allocation: the launches can be captured into a graph.
#pragma once
#include "evrep_common.h"
#include "evrep_detloss.hip"
#include "evrep_kd.h"
#include "evrep_f16.h"

#pragma clang fp contract(off)

namespace evrep {

constexpr int kDistillTile = EVREP_DISTILL_MAX_CLASSES;                // elements of p (and of tp) a workgroup holds: a whole row fits
constexpr int kCwStage = EVREP_CWD_STAGE;                                        // the longest row of a feature map that is staged in LDS
constexpr int kCwLevels = EVREP_CWD_MAX_LEVELS;                                        // distill_loss_cw reads s_feats[0 .. 2]

// rows of a tile: whole rows only, at most one per lane
__host__ __device__ inline int distill_tile_rows(int nc) {
    const int r = kDistillTile / nc;
    return r > kThreads ? kThreads : (r < 1 ? 1 : r);
}

// ------------------------------------------------------------------------------------------------------- class term, distilled
// grid (Gd, B), 256 threads; tile i of the image's rows belongs to workgroup i % Gd.  s_a / s_b hold, per element of the
// student's / the teacher's tile, first x / T, then exp(x / T - m), then the probability.
__global__ __launch_bounds__(kThreads) void k_detdistill_cls(const DetlossArgs t) {
    __shared__ double tmp[kWaves];
    __shared__ float s_p[kDistillTile];
    __shared__ double s_a[kDistillTile], s_b[kDistillTile];
    __shared__ double s_ms[kThreads], s_mt[kThreads], s_Zs[kThreads], s_Zt[kThreads], s_spt[kThreads];
    const int b = blockIdx.y, tid = threadIdx.x, nc = t.nc, A = t.A;
    const double tss = detloss_fold(t.tss_part, t.n_tss, tmp);
    const double norm = detloss_norm<true>(tss);
    const double sc = __ddiv_rn(t.wc, norm);
    const double ck = __dmul_rn(__dmul_rn(t.wc, t.k_class), t.T);      // d (wc * k_class * d_loss_cls) / d p = ck * (ps * sum(pt) - pt)
    const int rt = distill_tile_rows(nc), nt = (A + rt - 1) / rt;
    double s = 0.0, sd = 0.0;
    for (int tile = blockIdx.x; tile < nt; tile += gridDim.x) {
        const int a0 = tile * rt, na = A - a0 < rt ? A - a0 : rt, ne = na * nc;          // na <= kThreads, ne <= kDistillTile
        const size_t at0 = ((size_t)b * A + a0) * (size_t)nc;
        __syncthreads();                                               // the last tile's readers are done
        for (int i = tid; i < ne; i += kThreads) {
            const float p = t.p[at0 + i];
            s_p[i] = p;
            s_a[i] = __ddiv_rn((double)p, t.T);
            s_b[i] = __ddiv_rn((double)t.tp[at0 + i], t.T);
        }
        __syncthreads();
        if (tid < na) {                                                // m = max_k (x_k / T)
            const double *xa = s_a + tid * nc, *xb = s_b + tid * nc;
            double ms = xa[0], mt = xb[0];
            for (int k = 1; k < nc; ++k) { ms = dl_max(ms, xa[k]); mt = dl_max(mt, xb[k]); }
            s_ms[tid] = ms; s_mt[tid] = mt;
        }
        __syncthreads();
        for (int i = tid; i < ne; i += kThreads) {                     // e_k = exp(x_k / T - m)
            const int r = i / nc;
            s_a[i] = exp(__dsub_rn(s_a[i], s_ms[r]));
            s_b[i] = exp(__dsub_rn(s_b[i], s_mt[r]));
        }
        __syncthreads();
        if (tid < na) {                                                // Z = the e_k added left to right
            const double *ea = s_a + tid * nc, *eb = s_b + tid * nc;
            double Zs = 0.0, Zt = 0.0;
            for (int k = 0; k < nc; ++k) { Zs = __dadd_rn(Zs, ea[k]); Zt = __dadd_rn(Zt, eb[k]); }
            s_Zs[tid] = Zs; s_Zt[tid] = Zt;
        }
        __syncthreads();
        for (int i = tid; i < ne; i += kThreads) {                     // the probabilities and the element's KL term
            const int r = i / nc;
            const double ps = __ddiv_rn(s_a[i], s_Zs[r]), pt = __ddiv_rn(s_b[i], s_Zt[r]);
            s_a[i] = ps;
            s_b[i] = pt;
            sd = __dadd_rn(sd, kd_term(ps, pt));
        }
        __syncthreads();
        if (tid < na) {                                                // spt = the pt_k added left to right
            const double *pb = s_b + tid * nc;
            double spt = 0.0;
            for (int k = 0; k < nc; ++k) spt = __dadd_rn(spt, pb[k]);
            s_spt[tid] = spt;
        }
        __syncthreads();
        for (int i = tid; i < ne; i += kThreads) {
            const int r = i / nc, c = i - r * nc;
            const size_t ba = (size_t)b * A + a0 + r, at = at0 + i;
            const double p = (double)s_p[i], q = dl_target(t.ts, at, t.f32_t);
            const bool lab = t.fg[ba] != 0 && t.labels[ba] == (int64_t)c;
            double term, g;
            detloss_vfl(p, q, lab, t.grad != 0, term, g);
            s = __dadd_rn(s, term);
            if (t.grad) {
                const double gd = __dmul_rn(ck, __dsub_rn(__dmul_rn(s_a[i], s_spt[r]), s_b[i]));
                t.gs[at] = (float)__dadd_rn(__dmul_rn(sc, g), gd);
            }
        }
    }
    const double tot = detloss_block_sum(s, tmp), totd = detloss_block_sum(sd, tmp);
    if (tid == 0) {
        t.cls_part[(size_t)b * gridDim.x + blockIdx.x] = tot;
        t.dcls_part[(size_t)b * gridDim.x + blockIdx.x] = totd;
    }
}

// ------------------------------------------------------------------------------------------------- channel-wise distillation
struct CwdArgs {
    const void *s[kCwLevels], *t[kCwLevels];    // (N, C, H, W) each, of the element types sdt and tdt
    float *g[kCwLevels];                        // the same shape, or null
    int32_t hw[kCwLevels];                      // H * W
    int32_t rows[kCwLevels], row0[kCwLevels];   // N * C and the sum of the earlier levels'
    double gscale[kCwLevels], lscale[kCwLevels];   // tau / (N * C), tau^2 / (N * C)
    double tau;
    double *part;                               // scratch [rows of all levels]
    double *out;                                // [4]
    int32_t L, sdt, tdt;                        // EVREP_DT_* of s and of t
};

// element i of a row that starts `at` elements into a map of the element type dt (the same in every thread); the instance
// without 16-bit maps (kTyped false: both maps float32) is the plain load it always was
template <bool kTyped>
__device__ inline float cw_load(const void *map, size_t at, int i, int dt) {
    if (!kTyped || dt == EVREP_DT_F32) return static_cast<const float *>(map)[at + i];
    return widen16(static_cast<const uint16_t *>(map)[at + i], dt);
}

// the maximum over a workgroup of 256 (a > b ? a : b); valid in every thread; contains __syncthreads()
__device__ inline double cw_block_max(double v, double *tmp) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = dl_max(v, __shfl_xor(v, d, 64));
    if ((threadIdx.x & 63) == 0) tmp[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = tmp[0];
#pragma unroll
    for (int wv = 1; wv < kWaves; ++wv) r = dl_max(r, tmp[wv]);
    __syncthreads();
    return r;
}

// grid (rows of all levels), 256 threads; kTyped: either side is 16-bit
template <bool kTyped>
__global__ __launch_bounds__(kThreads) void k_detdistill_cw(const CwdArgs t) {
    __shared__ double tmp[kWaves];
    __shared__ float s_s[kCwStage], s_t[kCwStage];
    const int tid = threadIdx.x, row = blockIdx.x;
    int l = 0;
    if (t.L > 1 && row >= t.row0[1]) l = 1;
    if (t.L > 2 && row >= t.row0[2]) l = 2;
    const int n = t.hw[l];
    const size_t at = (size_t)(row - t.row0[l]) * (size_t)n;
    const void *S = t.s[l], *Tt = t.t[l];
    const bool staged = n <= kCwStage;
    const double ninf = -__longlong_as_double(0x7ff0000000000000ll);
    double ms = ninf, mt = ninf;
    for (int i = tid; i < n; i += kThreads) {
        const float a = cw_load<kTyped>(S, at, i, t.sdt), b = cw_load<kTyped>(Tt, at, i, t.tdt);
        if (staged) { s_s[i] = a; s_t[i] = b; }
        ms = dl_max(ms, __ddiv_rn((double)a, t.tau));
        mt = dl_max(mt, __ddiv_rn((double)b, t.tau));
    }
    ms = cw_block_max(ms, tmp);
    mt = cw_block_max(mt, tmp);
    double zs = 0.0, zt = 0.0;
    for (int i = tid; i < n; i += kThreads) {
        const float a = staged ? s_s[i] : cw_load<kTyped>(S, at, i, t.sdt), b = staged ? s_t[i] : cw_load<kTyped>(Tt, at, i, t.tdt);
        zs = __dadd_rn(zs, exp(__dsub_rn(__ddiv_rn((double)a, t.tau), ms)));
        zt = __dadd_rn(zt, exp(__dsub_rn(__ddiv_rn((double)b, t.tau), mt)));
    }
    const double lZs = log(detloss_block_sum(zs, tmp)), lZt = log(detloss_block_sum(zt, tmp));
    double kl = 0.0, spt = 0.0;
    for (int i = tid; i < n; i += kThreads) {
        const float a = staged ? s_s[i] : cw_load<kTyped>(S, at, i, t.sdt), b = staged ? s_t[i] : cw_load<kTyped>(Tt, at, i, t.tdt);
        const double ls = __dsub_rn(__dsub_rn(__ddiv_rn((double)a, t.tau), ms), lZs);
        const double lt = __dsub_rn(__dsub_rn(__ddiv_rn((double)b, t.tau), mt), lZt);
        const double pt = exp(lt);
        kl = __dadd_rn(kl, __dmul_rn(pt, __dsub_rn(lt, ls)));
        spt = __dadd_rn(spt, pt);
    }
    kl = detloss_block_sum(kl, tmp);
    if (tid == 0) t.part[row] = kl;
    if (t.g[l] == nullptr) return;                                     // (the same in every thread)
    spt = detloss_block_sum(spt, tmp);
    float *G = t.g[l] + at;
    const double gsc = t.gscale[l];
    for (int i = tid; i < n; i += kThreads) {
        const float a = staged ? s_s[i] : cw_load<kTyped>(S, at, i, t.sdt), b = staged ? s_t[i] : cw_load<kTyped>(Tt, at, i, t.tdt);
        const double ls = __dsub_rn(__dsub_rn(__ddiv_rn((double)a, t.tau), ms), lZs);
        const double lt = __dsub_rn(__dsub_rn(__ddiv_rn((double)b, t.tau), mt), lZt);
        G[i] = (float)__dmul_rn(gsc, __dsub_rn(__dmul_rn(exp(ls), spt), exp(lt)));
    }
}

// one workgroup of 256: out = [the sum, level 0, level 1, level 2]
__global__ __launch_bounds__(kThreads) void k_detdistill_cw_fold(const CwdArgs t) {
    __shared__ double tmp[kWaves];
    double lv[kCwLevels] = {0.0, 0.0, 0.0};
    for (int l = 0; l < t.L; ++l) lv[l] = __dmul_rn(detloss_fold(t.part + t.row0[l], (uint32_t)t.rows[l], tmp), t.lscale[l]);
    if (threadIdx.x == 0) {
        t.out[0] = __dadd_rn(__dadd_rn(lv[0], lv[1]), lv[2]);
        t.out[1] = lv[0];
        t.out[2] = lv[1];
        t.out[3] = lv[2];
    }
}

}  // namespace evrep
