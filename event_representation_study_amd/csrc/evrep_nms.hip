// evrep_nms.hip -- the detector's output: ev-YOLOv6's non_max_suppression (yolov6/utils/nms.py:59-129) with torchvision's CPU
// kernel (nms_kernel_impl) behind it, for the B images of a batch in ONE launch, one workgroup of sixteen waves per image.
//
//   (a) rows      first the boxes with obj > ct are listed in index order (one strided load per box), then one lane per LISTED
//                 box reads its classes -- every lane of a round has work, where a lane per box of the image would idle beside
//                 the few that pass: max(cls) > ct (a NaN among the classes makes torch.max NaN: no candidate), then the rows
//                 of the box -- multi_label: every class with fl32(cls * obj) > ct; otherwise the FIRST maximum of the products
//                 -- filtered by `classes`.  A row is the number i * C + c.  The counts of a round of 1024 boxes are scanned
//                 over the workgroup and every lane writes its rows behind its prefix: index order, no atomic.
//   (b) order     rank_pair_sort (evrep_ranksort.h) by the key ~rank_key(conf): stable, so equal scores keep index order
//                 (torchvision's stable descending sort), and the max_nms cut is a prefix (ties at the cut: lower row first).
//                 A row's box, score and class are recomputed from `pred` through its number; nothing decoded is stored.
//   (c) greedy    the sorted rows in rounds of 1024, one per lane, against a KEPT LIST in LDS (offset corners + area, at most
//                 max_det <= 1024 entries).  Every lane first tests its row against all rows kept in earlier rounds.  Then the
//                 sixteen waves take their turn in order: the wave resolves its survivors by a ballot loop -- the lowest
//                 surviving lane is kept, broadcasts its box, and the others test against it -- and after the turn's barrier
//                 all waves behind it test their rows against what it added, at once.  The pass ends at max_det kept rows.
//                 No n x n mask matrix.
//   (d) output    a kept row is written by its lane as the UN-offset [x1, y1, x2, y2, conf, cls]; the rows behind the last
//                 kept one are zero-filled and count[b] written: every output byte on every call.
//
// ROUNDING.  Every arithmetic statement of the reference is one float32 operation here, written with __fadd_rn / __fsub_rn /
// __fmul_rn / __fdiv_rn; that none of them is fused into a multiply-add (fl32(area_i + area_j) - fl32(w * h) must stay two
// roundings) is ensured twice: the library is compiled with -ffp-contract=off (build.FLAGS), and this file says so itself with
// the pragma below, which holds whatever flags a build passes.  w / 2 is the exact w * 0.5.  max / min are std::max / std::min
// as torchvision calls them, written as the comparisons they are (std::max(a, b) = a < b ? b : a), so a NaN coordinate takes
// the reference's way.  The IoU test is (double)ovr > iou_thres, strict; a NaN ovr (0 / 0) suppresses nothing.
//
// Plain C++ stores only, no floating-point atomic, nothing read back, no allocation: the launch can be captured into a graph.
#pragma once
#include "evrep_common.h"
#include "evrep_ranksort.h"

#pragma clang fp contract(off)

namespace evrep {

constexpr int kNmsMaxDet = EVREP_NMS_MAX_DET;
constexpr int kNmsMaskWords = EVREP_NMS_MAX_CLASSES / 32;
static_assert(kNmsMaxDet <= kDistThreads, "a round of the greedy pass can keep a row per lane");

struct NmsArgs {
    const float *pred;            // (B, N, 5 + C)
    float *det;                   // (B, max_det, 6)
    int32_t *count;               // (B)
    uint32_t *scratch;            // five arrays of B * R uint32: the pair sort's ka, ia, kb, ib, then the rows
    double iou_thres;
    int64_t R;                    // rows an image can have: N * C with multi, N otherwise
    float ct;
    int32_t B, N, C;
    int32_t multi;                // multi_label and C > 1
    int32_t agnostic;
    int32_t use_classes;          // class_mask holds the filter
    int32_t max_nms, max_det;
    uint32_t class_mask[kNmsMaskWords];
};

struct NmsRow {
    float x1, y1, x2, y2, conf, cls;
};

// the reference's row for the number r = i * C + c: xywh2xyxy, conf = cls * obj
__device__ inline NmsRow nms_row(const float *__restrict__ img, int C, uint32_t r) {
    const uint32_t i = r / (uint32_t)C, c = r - i * (uint32_t)C;
    const float *p = img + (size_t)i * (size_t)(5 + C);
    const float hw = __fmul_rn(p[2], 0.5f), hh = __fmul_rn(p[3], 0.5f);
    NmsRow o;
    o.x1 = __fsub_rn(p[0], hw);
    o.y1 = __fsub_rn(p[1], hh);
    o.x2 = __fadd_rn(p[0], hw);
    o.y2 = __fadd_rn(p[1], hh);
    o.conf = __fmul_rn(p[5 + c], p[4]);
    o.cls = (float)c;
    return o;
}

__device__ inline float nms_conf(const float *__restrict__ img, int C, uint32_t r) {
    const uint32_t i = r / (uint32_t)C, c = r - i * (uint32_t)C;
    const float *p = img + (size_t)i * (size_t)(5 + C);
    return __fmul_rn(p[5 + c], p[4]);
}

// the rows of box i (p: its 5 + C values): their count, the first one in `first`; all written to dst when it is given
__device__ inline uint32_t nms_box_rows(const float *__restrict__ p, const NmsArgs &a, const uint32_t *mask, uint32_t i, uint32_t *dst,
                                        uint32_t &first) {
    const float obj = p[4], ct = a.ct;
    if (!(obj > ct)) return 0u;
    const int C = a.C;
    bool nan = false;
    float mx = p[5];
#pragma unroll 8
    for (int c = 0; c < C; ++c) {
        const float v = p[5 + c];
        nan = nan || v != v;
        mx = v > mx ? v : mx;
    }
    if (nan || !(mx > ct)) return 0u;
    uint32_t k = 0;
    if (a.multi) {
#pragma unroll 8
        for (int c = 0; c < C; ++c) {
            const float conf = __fmul_rn(p[5 + c], obj);
            if (conf > ct && (!a.use_classes || ((mask[c >> 5] >> (c & 31)) & 1u))) {
                if (k == 0) first = i * (uint32_t)C + (uint32_t)c;
                if (dst) dst[k] = i * (uint32_t)C + (uint32_t)c;
                ++k;
            }
        }
    } else {
        int best = 0;
        float bv = __fmul_rn(p[5], obj);
        bool pnan = bv != bv;                     // inf * 0: torch.max returns the NaN, and NaN > ct drops the row
#pragma unroll 8
        for (int c = 1; c < C; ++c) {
            const float v = __fmul_rn(p[5 + c], obj);
            pnan = pnan || v != v;
            if (v > bv) {
                bv = v;
                best = c;
            }
        }
        if (!pnan && bv > ct && (!a.use_classes || ((mask[best >> 5] >> (best & 31)) & 1u))) {
            first = i * (uint32_t)C + (uint32_t)best;
            if (dst) dst[0] = first;
            k = 1;
        }
    }
    return k;
}

// does the kept row i suppress row j?  (nms_kernel_impl's inner statements, each its own rounding)
__device__ inline bool nms_suppresses(float ix1, float iy1, float ix2, float iy2, float iarea, float jx1, float jy1, float jx2, float jy2,
                                      float jarea, double iou_thres) {
    const float xx1 = ix1 < jx1 ? jx1 : ix1, yy1 = iy1 < jy1 ? jy1 : iy1;     // std::max(ix1, x1[j])
    const float xx2 = jx2 < ix2 ? jx2 : ix2, yy2 = jy2 < iy2 ? jy2 : iy2;     // std::min(ix2, x2[j])
    const float dw = __fsub_rn(xx2, xx1), dh = __fsub_rn(yy2, yy1);
    const float w = 0.0f < dw ? dw : 0.0f, h = 0.0f < dh ? dh : 0.0f;         // std::max(0, d)
    const float inter = __fmul_rn(w, h);
    const float ovr = __fdiv_rn(inter, __fsub_rn(__fadd_rn(iarea, jarea), inter));
    return (double)ovr > iou_thres;
}

// lane `src`'s value of v; src is the same in every lane of the wave (it comes from a ballot)
__device__ inline float nms_lane(float v, int src) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), __builtin_amdgcn_readfirstlane(src)));
}

// grid (B), 1024 threads
__global__ __launch_bounds__(kDistThreads) void k_nms(const NmsArgs a) {
    __shared__ RankSortLds lds;
    __shared__ float kx1[kNmsMaxDet], ky1[kNmsMaxDet], kx2[kNmsMaxDet], ky2[kNmsMaxDet], karea[kNmsMaxDet];
    __shared__ uint32_t s_mask[kNmsMaskWords];
    __shared__ int s_kept[kDistWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, C = a.C, N = a.N;
    const size_t stride = (size_t)(5 + C);
    const float *img = a.pred + (size_t)b * (size_t)N * stride;
    const size_t BR = (size_t)a.B * (size_t)a.R, o0 = (size_t)b * (size_t)a.R;
    uint32_t *const ka = a.scratch + o0, *const ia = a.scratch + BR + o0, *const kb = a.scratch + 2 * BR + o0;
    uint32_t *const ib = a.scratch + 3 * BR + o0, *const rows = a.scratch + 4 * BR + o0;
    float *det = a.det + (size_t)b * (size_t)a.max_det * 6u;

    if (tid < kNmsMaskWords) s_mask[tid] = a.class_mask[tid];
    __syncthreads();

    // (a) the boxes with obj > ct, in index order (their numbers in ka, which the sort only needs later; at most N <= R) ...
    uint32_t n_obj = 0;
    for (int i0 = 0; i0 < N; i0 += kDistThreads) {
        const int i = i0 + tid;
        const uint32_t pass = (i < N && img[(size_t)i * stride + 4] > a.ct) ? 1u : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<kDistWaves>(pass, lds.scan_tmp, &tot);
        if (pass) ka[n_obj + ex] = (uint32_t)i;
        n_obj += tot;
    }
    __syncthreads();
    // ... and their rows, a box per lane; n <= R: a box has at most C rows with multi, one otherwise
    uint32_t n = 0;
    for (uint32_t j0 = 0; j0 < n_obj; j0 += kDistThreads) {
        const uint32_t j = j0 + (uint32_t)tid;
        const uint32_t i = j < n_obj ? ka[j] : 0u;
        const float *p = img + (size_t)i * stride;
        uint32_t first = 0;
        const uint32_t k = j < n_obj ? nms_box_rows(p, a, s_mask, i, nullptr, first) : 0u;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<kDistWaves>(k, lds.scan_tmp, &tot);
        if (k == 1) rows[n + ex] = first;
        else if (k > 1) nms_box_rows(p, a, s_mask, i, rows + n + ex, first);
        n += tot;
    }
    __syncthreads();                                      // the rows are in place for every wave of this workgroup

    // (b) conf descending, ties by index
    rank_pair_sort([img, C, rows](int64_t q) { return ~rank_key(nms_conf(img, C, rows[q])); }, (int64_t)n, ka, ia, kb, ib, lds);
    const uint32_t m = n < (uint32_t)a.max_nms ? n : (uint32_t)a.max_nms;

    // (c) the greedy pass
    int K = 0;                                            // rows kept so far (uniform)
    for (uint32_t q0 = 0; q0 < m && K < a.max_det; q0 += kDistThreads) {
        const uint32_t q = q0 + (uint32_t)tid;
        bool alive = q < m;
        NmsRow row = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        float ox1 = 0.0f, oy1 = 0.0f, ox2 = 0.0f, oy2 = 0.0f, area = 0.0f;
        if (alive) {
            row = nms_row(img, C, rows[ib[q]]);
            const float off = a.agnostic ? __fmul_rn(row.cls, 0.0f) : __fmul_rn(row.cls, 4096.0f);
            ox1 = __fadd_rn(row.x1, off);
            oy1 = __fadd_rn(row.y1, off);
            ox2 = __fadd_rn(row.x2, off);
            oy2 = __fadd_rn(row.y2, off);
            area = __fmul_rn(__fsub_rn(ox2, ox1), __fsub_rn(oy2, oy1));
        }
        for (int k = 0; k < K; ++k) {
            if (__ballot(alive) == 0ull) break;
            if (alive && nms_suppresses(kx1[k], ky1[k], kx2[k], ky2[k], karea[k], ox1, oy1, ox2, oy2, area, a.iou_thres)) alive = false;
        }
        int seen = K;                                     // kept entries this lane's row has been tested against
        for (int w = 0; w < kDistWaves; ++w) {
            if (wave == w) {
                int Kw = seen;                            // K + what the waves in front kept in this round
                uint64_t live = __ballot(alive);
                while (live != 0ull && Kw < a.max_det) {
                    const int lead = __ffsll((unsigned long long)live) - 1;
                    const float lx1 = nms_lane(ox1, lead), ly1 = nms_lane(oy1, lead), lx2 = nms_lane(ox2, lead);
                    const float ly2 = nms_lane(oy2, lead), larea = nms_lane(area, lead);
                    if (lane == lead) {
                        kx1[Kw] = ox1; ky1[Kw] = oy1; kx2[Kw] = ox2; ky2[Kw] = oy2; karea[Kw] = area;      // Kw < max_det <= kNmsMaxDet
                        float *d = det + (size_t)Kw * 6u;
                        gstore_f32(d + 0, row.x1); gstore_f32(d + 1, row.y1); gstore_f32(d + 2, row.x2); gstore_f32(d + 3, row.y2);
                        gstore_f32(d + 4, row.conf); gstore_f32(d + 5, row.cls);
                        alive = false;
                    } else if (alive && nms_suppresses(lx1, ly1, lx2, ly2, larea, ox1, oy1, ox2, oy2, area, a.iou_thres)) {
                        alive = false;
                    }
                    ++Kw;
                    live = __ballot(alive);
                }
                if (lane == 0) s_kept[w] = Kw;            // a slot per turn: read below by everyone, rewritten a round later
            }
            __syncthreads();
            const int now = s_kept[w];
            if (wave > w) {                               // the waves behind test against what this turn added, all at once
                for (int k = seen; k < now; ++k) {
                    if (__ballot(alive) == 0ull) break;
                    if (alive && nms_suppresses(kx1[k], ky1[k], kx2[k], ky2[k], karea[k], ox1, oy1, ox2, oy2, area, a.iou_thres)) alive = false;
                }
            }
            seen = now;
            if (now >= a.max_det) break;                  // (uniform: every thread read the same slot)
        }
        K = seen;
    }

    // (d) the rows behind the last kept one, and the count
    for (int e = K * 6 + tid; e < a.max_det * 6; e += kDistThreads) gstore_f32(det + e, 0.0f);
    if (tid == 0) a.count[b] = K;
}

}  // namespace evrep
