// evrep_deteval.hip -- scoring the detections: the statistics step of ev-YOLOv6's validation loop (yolov6/core/evaler.py:206-258
// with yolov6/utils/metrics.py's process_batch and ConfusionMatrix.process_batch behind it) for the B images of a batch in ONE
// launch, one workgroup of sixteen waves per image.  include/evrep.h states the rules with evrep_det_match.
//
//   (a) labels    the workgroup sweeps `targets` in rounds of 1024 rows, a row per lane; the rows of its image (column 0 == b)
//                 are counted by a scan over the workgroup, so they are listed in array order without an atomic.  A listed row
//                 is taken to the source frame (xywh2xyxy, x *= W, y *= H, scale_coords), written to tbox and kept in LDS as
//                 box, area and class -- the first EVREP_DETEVAL_MAX_LABELS of them; an image with more gets all-false rows.
//                 Workgroup 0 also zero-fills the tbox rows that belong to no image.
//   (b) score     a lane per detection (max_det <= 1024): its box through scale_coords (written to detn), then ONE walk over
//                 the labels in LDS (every lane reads the same label: a broadcast), keeping k* / iou* among the labels of
//                 its class and, for the confusion matrix, the best label of any class above iou_thres.  A later label
//                 replaces an earlier one only with a GREATER IoU: the lowest label index wins a tie.
//   (c) claim     claim[k][i] = the lowest detection index with k* == k and iou* >= iouv[i], by an LDS atomicMin; correct[j][i]
//                 is "I hold my label's claim".  No sort.
//   (d) matrix    win[k] = max over the detections whose best label is k of (rank_key(iou) << 32 | ~j), a 64-bit LDS atomicMax:
//                 the greatest IoU, the lowest detection index among equals.  The reference's three kinds of update follow:
//                 counted in an LDS copy of the matrix when it has at most 1024 cells (nc <= 31) and added to the caller's
//                 with one global 64-bit integer atomic per non-zero cell, else a global atomic per update.
//
// ROUNDING.  Every arithmetic statement of the reference is one float32 operation, written with __fadd_rn / __fsub_rn /
// __fmul_rn / __fdiv_rn; that none is fused into a multiply-add is ensured twice: the library is compiled with
// -ffp-contract=off (build.FLAGS), and this file says so itself with the pragma below.  w / 2 is the exact w * 0.5.  min / max /
// clamp are the comparisons they are; torch's propagate a NaN where these do not, which changes no result: a box with a NaN
// corner has a NaN area, so its IoU is NaN whatever the intersection is, and a NaN IoU matches nothing.
//
// Every loop ends at a value the host passed or at a count capped at 1024.  Plain C++ stores, integer atomics only, nothing
// read back, no allocation, no scratch: the launch can be captured into a graph.
#pragma once
#include "evrep_common.h"
#include "evrep_ranksort.h"

#pragma clang fp contract(off)

namespace evrep {

constexpr int kDetevalMaxLabels = EVREP_DETEVAL_MAX_LABELS;
constexpr int kDetevalMaxT = EVREP_DETEVAL_MAX_T;
constexpr int kDetevalLocalCells = 1024;                              // a matrix of up to this many cells is counted in LDS first
static_assert(kDetevalMaxLabels <= kDistThreads && EVREP_NMS_MAX_DET <= kDistThreads, "a lane per label and a lane per detection");

struct DetevalArgs {
    const float *det;             // (B, max_det, 6)
    const int32_t *count;         // (B)
    const float *targets;         // (n_t, 6)
    const float *geom;            // (B, 5): pad_x, pad_y, gain, w0, h0; not read in native mode
    unsigned long long *matrix;   // (nc + 1) * (nc + 1) or null
    uint8_t *correct;             // (B, max_det, T)
    float *detn;                  // (B, max_det, 6) or null
    float *tbox;                  // (n_t, 4) or null
    int32_t *n_labels;            // (B)
    uint32_t *status;             // (B)
    int64_t n_t;
    float iouv[kDetevalMaxT];
    float img_h, img_w, conf, iou_thres;
    int32_t B, max_det, T, nc;
    int32_t native, skip_empty;
};

// clamp_(0, hi) as two comparisons: a NaN stays
__device__ inline float deteval_clamp(float v, float hi) { return v < 0.0f ? 0.0f : (v > hi ? hi : v); }

// scale_coords for one coordinate: subtract the pad, divide by gain[0], clamp to the frame
__device__ inline float deteval_scale(float v, float pad, float gain, float hi) {
    return deteval_clamp(__fdiv_rn(__fsub_rn(v, pad), gain), hi);
}

// int(c) when it lies in [0, nc), else -1 (a NaN fails both comparisons)
__device__ inline int deteval_class(float c, int nc) { return (c > -1.0f && c < (float)nc) ? (int)c : -1; }

// grid (B), 1024 threads
__global__ __launch_bounds__(kDistThreads) void k_det_match(const DetevalArgs a) {
    __shared__ float4 s_box[kDetevalMaxLabels];                        // a label's native-space corners
    __shared__ float2 s_ac[kDetevalMaxLabels];                         // its area and class
    __shared__ uint32_t s_claim[kDetevalMaxLabels * kDetevalMaxT];     // [k * T + i]: the first claimant
    __shared__ unsigned long long s_win[kDetevalMaxLabels];
    __shared__ float s_dcls[EVREP_NMS_MAX_DET];
    __shared__ uint32_t s_cells[kDetevalLocalCells];
    __shared__ uint32_t s_scan[kDistWaves];
    __shared__ uint32_t s_status, s_any;
    const int tid = threadIdx.x, b = blockIdx.x, T = a.T, nc = a.nc;
    const float fb = (float)b, fB = (float)a.B;
    float pad_x = 0.0f, pad_y = 0.0f, gain = 1.0f, w0 = 0.0f, h0 = 0.0f;
    if (!a.native) {
        const float *g = a.geom + (size_t)b * 5u;
        pad_x = g[0]; pad_y = g[1]; gain = g[2]; w0 = g[3]; h0 = g[4];
    }
    if (tid == 0) {
        s_status = 0u;
        s_any = 0u;
    }

    // (a) the labels of this image, in array order (block_exclusive_scan's barriers also publish the two words above)
    uint32_t n = 0;
    for (int64_t r0 = 0; r0 < a.n_t; r0 += kDistThreads) {
        const int64_t r = r0 + tid;
        const bool in = r < a.n_t;
        const float *t = a.targets + (size_t)(in ? r : 0) * 6u;
        const float t0 = in ? t[0] : 0.0f;
        const bool mine = in && t0 == fb;
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<kDistWaves>(mine ? 1u : 0u, s_scan, &tot);
        if (mine) {
            float x1 = t[2], y1 = t[3], x2 = t[4], y2 = t[5];
            if (!a.native) {
                const float hw = __fmul_rn(x2, 0.5f), hh = __fmul_rn(y2, 0.5f), cx = x1, cy = y1;
                x1 = deteval_scale(__fmul_rn(__fsub_rn(cx, hw), a.img_w), pad_x, gain, w0);
                y1 = deteval_scale(__fmul_rn(__fsub_rn(cy, hh), a.img_h), pad_y, gain, h0);
                x2 = deteval_scale(__fmul_rn(__fadd_rn(cx, hw), a.img_w), pad_x, gain, w0);
                y2 = deteval_scale(__fmul_rn(__fadd_rn(cy, hh), a.img_h), pad_y, gain, h0);
            }
            if (a.tbox) {
                float *o = a.tbox + (size_t)r * 4u;                    // r < n_t
                gstore_f32(o + 0, x1); gstore_f32(o + 1, y1); gstore_f32(o + 2, x2); gstore_f32(o + 3, y2);
            }
            const uint32_t pos = n + ex;
            if (pos < (uint32_t)kDetevalMaxLabels) {
                s_box[pos] = make_float4(x1, y1, x2, y2);
                s_ac[pos] = make_float2(__fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1)), t[1]);
            }
        } else if (b == 0 && in && a.tbox && !(t0 >= 0.0f && t0 < fB && t0 == truncf(t0))) {
            float *o = a.tbox + (size_t)r * 4u;                        // a row of no image: zeros
            gstore_f32(o + 0, 0.0f); gstore_f32(o + 1, 0.0f); gstore_f32(o + 2, 0.0f); gstore_f32(o + 3, 0.0f);
        }
        n += tot;
    }
    const bool over = n > (uint32_t)kDetevalMaxLabels;
    const int nl = over ? 0 : (int)n;                                  // <= 1024
    const int c_in = a.count[b];
    const int cnt = c_in < 0 ? 0 : (c_in > a.max_det ? a.max_det : c_in);
    const bool cm = a.matrix != nullptr && !over && !(a.skip_empty && cnt == 0);
    uint32_t st = (over ? EVREP_DETEVAL_ST_LABEL_OVERFLOW : 0u) | (c_in != cnt ? EVREP_DETEVAL_ST_BAD_COUNT : 0u);

    for (int e = tid; e < nl * T; e += kDistThreads) s_claim[e] = 0xFFFFFFFFu;   // nl * T <= 1024 * 16
    if (tid < nl) s_win[tid] = 0ull;
    const int cells = (nc + 1) * (nc + 1);                            // nc <= 4096: no overflow
    const bool local = cm && cells <= kDetevalLocalCells;
    if (local && tid < cells) s_cells[tid] = 0u;                       // cells <= 1024 threads
    __syncthreads();                                                  // the labels and the empty tables are in place

    // (b) a detection per lane
    int kb = -1, ck = -1;
    float best = 0.0f, cbest = 0.0f, dconf = 0.0f, dcls = 0.0f;
    bool part = false;
    if (tid < cnt) {
        const float *d = a.det + ((size_t)b * (size_t)a.max_det + (size_t)tid) * 6u;
        float x1 = d[0], y1 = d[1], x2 = d[2], y2 = d[3];
        dconf = d[4];
        dcls = d[5];
        if (!a.native) {
            x1 = deteval_scale(x1, pad_x, gain, w0);
            y1 = deteval_scale(y1, pad_y, gain, h0);
            x2 = deteval_scale(x2, pad_x, gain, w0);
            y2 = deteval_scale(y2, pad_y, gain, h0);
        }
        s_dcls[tid] = dcls;                                            // tid < cnt <= max_det <= EVREP_NMS_MAX_DET
        if (a.detn) {
            float *o = a.detn + ((size_t)b * (size_t)a.max_det + (size_t)tid) * 6u;
            gstore_f32(o + 0, x1); gstore_f32(o + 1, y1); gstore_f32(o + 2, x2); gstore_f32(o + 3, y2);
            gstore_f32(o + 4, dconf); gstore_f32(o + 5, dcls);
        }
        const float area_d = __fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1));
        part = cm && dconf > a.conf;
        for (int k = 0; k < nl; ++k) {
            const float4 L = s_box[k];
            const float2 ac = s_ac[k];
            const float xx2 = L.z < x2 ? L.z : x2, yy2 = L.w < y2 ? L.w : y2;         // min
            const float xx1 = L.x < x1 ? x1 : L.x, yy1 = L.y < y1 ? y1 : L.y;         // max
            const float dw = __fsub_rn(xx2, xx1), dh = __fsub_rn(yy2, yy1);
            const float w = dw < 0.0f ? 0.0f : dw, h = dh < 0.0f ? 0.0f : dh;         // clamp(0)
            const float inter = __fmul_rn(w, h);
            const float iou = __fdiv_rn(inter, __fsub_rn(__fadd_rn(ac.x, area_d), inter));
            if (ac.y == dcls && iou == iou && (kb < 0 || iou > best)) {
                kb = k;
                best = iou;
            }
            if (part && iou > a.iou_thres && (ck < 0 || iou > cbest)) {
                ck = k;
                cbest = iou;
            }
        }
        // (c) kb < nl, i < T: inside the nl * T entries initialised above
        if (kb >= 0) {
            for (int i = 0; i < T; ++i)
                if (best >= a.iouv[i]) atomicMin(&s_claim[kb * T + i], (uint32_t)tid);
        }
        if (ck >= 0) {
            atomicMax(&s_win[ck], ((unsigned long long)rank_key(cbest) << 32) | (unsigned long long)(~(uint32_t)tid));
            s_any = 1u;
        }
    }
    __syncthreads();

    if (tid < a.max_det) {
        uint8_t *o = a.correct + ((size_t)b * (size_t)a.max_det + (size_t)tid) * (size_t)T;
        for (int i = 0; i < T; ++i) o[i] = (kb >= 0 && best >= a.iouv[i] && s_claim[kb * T + i] == (uint32_t)tid) ? 1 : 0;
        if (a.detn && tid >= cnt) {
            float *z = a.detn + ((size_t)b * (size_t)a.max_det + (size_t)tid) * 6u;
            for (int e = 0; e < 6; ++e) gstore_f32(z + e, 0.0f);
        }
    }

    // (d) the confusion matrix; every index below is row * (nc + 1) + col with 0 <= row, col <= nc: inside the cells
    if (cm) {
        const size_t side = (size_t)nc + 1u;
        const auto add = [&](size_t cell) {
            if (local) atomicAdd(&s_cells[cell], 1u);
            else atomicAdd(a.matrix + cell, 1ull);
        };
        if (tid < nl) {
            const unsigned long long w = s_win[tid];
            const int gc = deteval_class(s_ac[tid].y, nc);
            const int row = w != 0ull ? deteval_class(s_dcls[~(uint32_t)w], nc) : nc;      // ~low word = a lane that had tid < cnt
            if (gc < 0 || row < 0) st |= EVREP_DETEVAL_ST_BAD_CLASS;
            else add((size_t)row * side + (size_t)gc);
        }
        if (part && s_any != 0u && !(ck >= 0 && ~(uint32_t)s_win[ck] == (uint32_t)tid)) {
            const int dc = deteval_class(dcls, nc);
            if (dc < 0) st |= EVREP_DETEVAL_ST_BAD_CLASS;
            else add((size_t)dc * side + (size_t)nc);
        }
    }
    if (st != 0u) atomicOr(&s_status, st);
    __syncthreads();
    if (local && tid < cells && s_cells[tid] != 0u) atomicAdd(a.matrix + tid, (unsigned long long)s_cells[tid]);
    if (tid == 0) {
        a.status[b] = s_status;
        a.n_labels[b] = (int32_t)n;
    }
}

}  // namespace evrep
