// evrep_capi_detin.hip -- the extern "C" surface, part 10: the detector.  Argument checks and the launches of each entry
// point; no plan, no allocation, no wait for the device.  The families, in the file's order:
//   input batch        evrep_detector_input, and for frames of different sizes evrep_resize_tap_tables and
//                      evrep_detector_input_frames (evrep_detin.hip, evrep_detin_frames.hip)
//   detections         evrep_nms, the batched non_max_suppression (evrep_nms.hip)
//   scoring            evrep_det_match against the labels (evrep_deteval.hip); evrep_det_ap_gather, evrep_det_ap (evrep_detap.hip)
//   training targets   evrep_det_targets_pad, evrep_tal_assign (evrep_assign.hip); evrep_atss_assign of the warm-up epochs (evrep_atss.hip)
//   loss terms         evrep_detloss_decode, evrep_detloss with the gradients (evrep_detloss.hip)
//   distillation       evrep_detloss_distill, evrep_detloss_cwd and its typed form (evrep_detdistill.hip); evrep_cast16_host,
//                      the 16-bit maps' conversions on the host
//   head               evrep_dethead_predict / _train / _train_backward and their typed forms (evrep_dethead.hip)
//   parameter update   evrep_train_step, evrep_ema_update (evrep_step.hip)
#include <limits.h>

#include "evrep_capi_shared.h"
#include "evrep_detin_frames.hip"
#include "evrep_nms.hip"
#include "evrep_deteval.hip"
#include "evrep_detap.hip"
#include "evrep_assign.hip"
#include "evrep_atss.hip"
#include "evrep_detloss.hip"
#include "evrep_detdistill.hip"
#include "evrep_dethead.hip"
#include "evrep_step.hip"

using namespace evrep;
using evrep_host::hip_check;

template <typename T>
static int detin_launch(const DetinArgs<double> &d, const void *rep, int32_t B, hipStream_t stream) {
    DetinArgs<T> a;
    a.src = static_cast<const T *>(rep);
    a.ystart = d.ystart; a.ycount = d.ycount; a.xstart = d.xstart; a.xcount = d.xcount; a.ywt = d.ywt; a.xwt = d.xwt;
    a.pad = d.pad; a.flags = d.flags; a.warp = d.warp; a.out = d.out;
    a.H = d.H; a.W = d.W; a.C = d.C; a.nh = d.nh; a.nw = d.nw; a.Tt = d.Tt; a.S = d.S; a.top = d.top; a.left = d.left;
    a.scale = d.scale;
    const int P = kThreads / ((d.C + kDetinGroup - 1) / kDetinGroup);   // pixels of a workgroup (evrep_detin.hip)
    const dim3 grid((unsigned)(((size_t)d.S * d.S + P - 1) / P), (unsigned)B);
    k_detector_input<T><<<grid, kThreads, 0, stream>>>(a);
    LAUNCH_CHECK("k_detector_input");
    return EVREP_OK;
}

// The claim arrays, what both assigners keep per (image, anchor) at the head of their scratch: the rows that claim the anchor
// (cnt), the lowest of them (first), the assigned row, and one double (val: TalArgs' metric, AtssArgs' score value).
template <typename Args>
static void claim_layout(Carver &c, int32_t B, int32_t A, Args *t) {
    const size_t ba = (size_t)B * (size_t)A;
    uint32_t *cnt = c.take<uint32_t>(ba * 4);
    uint32_t *first = c.take<uint32_t>(ba * 4);
    int32_t *row = c.take<int32_t>(ba * 4);
    double *val = c.take<double>(ba * 8);
    if (t) {
        t->cnt = cnt; t->first = first; t->row = row; t->val = val;
    }
}

extern "C" {

int evrep_detector_input(const void *rep, int32_t rep_dtype, int32_t B, int32_t H, int32_t W, int32_t C, int32_t nh, int32_t nw,
                         int32_t T, const int32_t *ystart, const int32_t *ycount, const double *ywt, const int32_t *xstart,
                         const int32_t *xcount, const double *xwt, int32_t S, int32_t top, int32_t left, const double *pad,
                         const uint32_t *flags, const int32_t *warp, float scale, float *out, void *stream_) {
    if (!is_float_dtype(rep_dtype)) return EVREP_EINVAL;
    if (B <= 0 || B > 65535 || C < 1 || C > EVREP_MAX_CHANNELS) return EVREP_EINVAL;
    if (H < 1 || W < 1 || H > EVREP_MAX_DIM || W > EVREP_MAX_DIM || S < 1 || S > EVREP_MAX_DIM) return EVREP_EINVAL;
    if (nh < 1 || nw < 1 || top < 0 || left < 0 || nh > S - top || nw > S - left || T < 1 || T > EVREP_MAX_DIM) return EVREP_EINVAL;
    if (!(scale == scale)) return EVREP_EINVAL;   // NaN
    if (bad_ptr(rep, rep_dtype == EVREP_F64 ? 8 : 4) || bad_ptr(out, 4) || bad_ptr(pad, 8)) return EVREP_EINVAL;
    if (bad_ptr(ystart, 4) || bad_ptr(ycount, 4) || bad_ptr(ywt, 8) || bad_ptr(xstart, 4) || bad_ptr(xcount, 4) || bad_ptr(xwt, 8))
        return EVREP_EINVAL;
    if (flags ? (bad_ptr(flags, 4) || bad_ptr(warp, 4)) : warp != nullptr) return EVREP_EINVAL;   // the two come together
    DetinArgs<double> d;
    memset(&d, 0, sizeof(d));
    d.ystart = ystart; d.ycount = ycount; d.xstart = xstart; d.xcount = xcount; d.ywt = ywt; d.xwt = xwt;
    d.pad = pad; d.flags = flags; d.warp = warp; d.out = out;
    d.H = H; d.W = W; d.C = C; d.nh = nh; d.nw = nw; d.Tt = T; d.S = S; d.top = top; d.left = left;
    d.scale = scale;
    hipStream_t stream = as_stream(stream_);
    if (rep_dtype == EVREP_F64) return detin_launch<double>(d, rep, B, stream);
    return detin_launch<float>(d, rep, B, stream);
}

int evrep_resize_tap_tables(const int32_t *axes, int32_t n_axes, int32_t max_dst, int32_t *start, int32_t *count, double *weights,
                            int64_t n_rows, int64_t n_wt, void *stream_) {
    if (n_axes < 1 || max_dst < 1 || max_dst > EVREP_MAX_DIM) return EVREP_EINVAL;
    if (n_rows < 1 || n_wt < 1 || n_rows > INT32_MAX || n_wt > INT32_MAX) return EVREP_EINVAL;
    if (bad_ptr(axes, 4) || bad_ptr(start, 4) || bad_ptr(count, 4) || bad_ptr(weights, 8)) return EVREP_EINVAL;
    TapTableArgs a;
    a.axes = axes; a.start = start; a.count = count; a.wt = weights; a.n_rows = n_rows; a.n_wt = n_wt; a.n_axes = n_axes;
    const dim3 grid((unsigned)n_axes, (unsigned)((max_dst + kThreads - 1) / kThreads));
    k_resize_tap_tables<<<grid, kThreads, 0, as_stream(stream_)>>>(a);
    LAUNCH_CHECK("k_resize_tap_tables");
    return EVREP_OK;
}

// frames_dev: the device copy of the B frame descriptors
static inline size_t detin_frames_bytes(int32_t B) { return (size_t)B * sizeof(evrep_detin_frame); }

size_t evrep_detector_input_frames_scratch_bytes(int32_t B) {
    return (B < 1 || B > 65535) ? 0 : detin_frames_bytes(B);
}

// offset >= 0 and [offset, offset + n * per) inside [0, limit)
static inline bool run_inside(int32_t off, int32_t n, int32_t per, int64_t limit) {
    return off >= 0 && (int64_t)off + (int64_t)n * per <= limit;
}

int evrep_detector_input_frames(const evrep_detin_frame *frames, int32_t B, int32_t rep_dtype, int32_t C, int32_t S,
                                const int32_t *start, const int32_t *count, const double *weights, int64_t n_rows, int64_t n_wt,
                                const double *pad, const int32_t *warp, float scale, void *frames_dev, float *out, void *stream_) {
    if (!is_float_dtype(rep_dtype)) return EVREP_EINVAL;
    if (B <= 0 || B > 65535 || C < 1 || C > EVREP_MAX_CHANNELS || S < 1 || S > EVREP_MAX_DIM) return EVREP_EINVAL;
    if (n_rows < 1 || n_wt < 1 || n_rows > INT32_MAX || n_wt > INT32_MAX) return EVREP_EINVAL;
    if (!(scale == scale)) return EVREP_EINVAL;   // NaN
    if (bad_ptr(frames, 8) || bad_ptr(frames_dev, 8) || bad_ptr(out, 4) || bad_ptr(pad, 8)) return EVREP_EINVAL;
    if (bad_ptr(start, 4) || bad_ptr(count, 4) || bad_ptr(weights, 8)) return EVREP_EINVAL;
    const uintptr_t elem = rep_dtype == EVREP_F64 ? 8 : 4;
    const auto dim = [](int32_t v) { return v >= 1 && v <= EVREP_MAX_DIM; };
    bool warps = false;
    for (int32_t b = 0; b < B; ++b) {
        const evrep_detin_frame &f = frames[b];
        if (bad_ptr(f.src, elem)) return EVREP_EINVAL;
        if (!dim(f.H) || !dim(f.W) || !dim(f.rh) || !dim(f.rw) || !dim(f.nh) || !dim(f.nw) || !dim(f.T1)) return EVREP_EINVAL;
        if (f.T2 < 0 || f.T2 > EVREP_MAX_DIM) return EVREP_EINVAL;
        if (f.top < 0 || f.left < 0 || f.nh > S - f.top || f.nw > S - f.left) return EVREP_EINVAL;
        if (!run_inside(f.row1, f.rh, 1, n_rows) || !run_inside(f.col1, f.rw, 1, n_rows)) return EVREP_EINVAL;
        if (!run_inside(f.wrow1, f.rh, f.T1, n_wt) || !run_inside(f.wcol1, f.rw, f.T1, n_wt)) return EVREP_EINVAL;
        if (f.T2 == 0) {
            if (f.nh != f.rh || f.nw != f.rw) return EVREP_EINVAL;
        } else {
            if (!run_inside(f.row2, f.nh, 1, n_rows) || !run_inside(f.col2, f.nw, 1, n_rows)) return EVREP_EINVAL;
            if (!run_inside(f.wrow2, f.nh, f.T2, n_wt) || !run_inside(f.wcol2, f.nw, f.T2, n_wt)) return EVREP_EINVAL;
        }
        if (f.flags & ~(EVREP_DETIN_WARP | EVREP_DETIN_FLIPUD | EVREP_DETIN_FLIPLR)) return EVREP_EINVAL;
        warps = warps || (f.flags & EVREP_DETIN_WARP) != 0u;
    }
    if (warps ? bad_ptr(warp, 4) : warp != nullptr) return EVREP_EINVAL;   // the flag and the tables come together
    hipStream_t stream = as_stream(stream_);
    int rc = hip_check(hipMemcpyAsync(frames_dev, frames, detin_frames_bytes(B), hipMemcpyHostToDevice, stream),
                       "hipMemcpyAsync(frames)");
    if (rc != EVREP_OK) return rc;
    const int P = kThreads / ((C + kDetinGroup - 1) / kDetinGroup);   // pixels of a workgroup (evrep_detin.hip)
    const dim3 grid((unsigned)(((size_t)S * S + P - 1) / P), (unsigned)B);
    const auto fill = [&](auto &a) {
        a.frames = static_cast<const evrep_detin_frame *>(frames_dev);
        a.tstart = start; a.tcount = count; a.twt = weights; a.pad = pad; a.warp = warp; a.out = out;
        a.n_rows = n_rows; a.n_wt = n_wt; a.C = C; a.S = S; a.scale = scale;
    };
    if (rep_dtype == EVREP_F64) {
        DetinFramesArgs<double> a;
        fill(a);
        k_detector_input_frames<double><<<grid, kThreads, 0, stream>>>(a);
    } else {
        DetinFramesArgs<float> a;
        fill(a);
        k_detector_input_frames<float><<<grid, kThreads, 0, stream>>>(a);
    }
    LAUNCH_CHECK("k_detector_input_frames");
    return EVREP_OK;
}

// the rows an image can have, every box a candidate under every class
static inline int64_t nms_rows(int32_t N, int32_t C, uint32_t flags) {
    return ((flags & EVREP_NMS_MULTI_LABEL) && C > 1) ? (int64_t)N * C : (int64_t)N;
}

int evrep_nms(const float *pred, int32_t B, int32_t N, int32_t C, float conf_thres, double iou_thres, uint32_t flags,
              const int32_t *classes_host, int32_t n_classes, int32_t max_nms, int32_t max_det, float *det, int32_t *count,
              void *scratch, void *stream_) {
    if (B < 1 || B > 65535 || N < 1 || C < 1 || C > EVREP_NMS_MAX_CLASSES || (int64_t)N * C > EVREP_NMS_MAX_ROWS) return EVREP_EINVAL;
    if (max_det < 1 || max_det > EVREP_NMS_MAX_DET || max_nms < 1) return EVREP_EINVAL;
    if (!(conf_thres >= 0.0f && conf_thres <= 1.0f) || !(iou_thres >= 0.0 && iou_thres <= 1.0)) return EVREP_EINVAL;   // (NaN fails)
    if (flags & ~(uint32_t)(EVREP_NMS_MULTI_LABEL | EVREP_NMS_AGNOSTIC)) return EVREP_EINVAL;
    if (n_classes < -1 || n_classes > EVREP_NMS_MAX_ROWS || (n_classes > 0 && bad_ptr(classes_host, 4))) return EVREP_EINVAL;
    if (bad_ptr(pred, 4) || bad_ptr(det, 4) || bad_ptr(count, 4) || bad_ptr(scratch, 16)) return EVREP_EINVAL;
    const int64_t R = nms_rows(N, C, flags);
    if (5 * (((int64_t)B * R + 3) / 4) > EVREP_RANK_MAX_TOTAL) return EVREP_EINVAL;
    NmsArgs a;
    memset(&a, 0, sizeof(a));
    a.pred = pred; a.det = det; a.count = count; a.scratch = static_cast<uint32_t *>(scratch);
    a.iou_thres = iou_thres; a.R = R; a.ct = conf_thres;
    a.B = B; a.N = N; a.C = C;
    a.multi = ((flags & EVREP_NMS_MULTI_LABEL) && C > 1) ? 1 : 0;
    a.agnostic = (flags & EVREP_NMS_AGNOSTIC) ? 1 : 0;
    a.use_classes = n_classes >= 0 ? 1 : 0;
    a.max_nms = max_nms; a.max_det = max_det;
    for (int32_t k = 0; k < n_classes; ++k) {
        const int32_t c = classes_host[k];
        if (c >= 0 && c < C) a.class_mask[c >> 5] |= 1u << (c & 31);
    }
    k_nms<<<(unsigned)B, kDistThreads, 0, as_stream(stream_)>>>(a);
    LAUNCH_CHECK("k_nms");
    return EVREP_OK;
}

int evrep_det_match(const float *det, const int32_t *count, int32_t B, int32_t max_det, const float *targets, int64_t n_t,
                    const float *geom, int32_t img_h, int32_t img_w, const float *iouv_host, int32_t T, uint32_t flags,
                    int64_t *matrix, int32_t nc, float conf, float iou_thres, uint8_t *correct, float *detn, float *tbox,
                    int32_t *n_labels, uint32_t *status, void *stream_) {
    if (B < 1 || B > 65535 || max_det < 1 || max_det > EVREP_NMS_MAX_DET) return EVREP_EINVAL;
    if (n_t < 0 || n_t > EVREP_DETEVAL_MAX_TARGETS || T < 1 || T > EVREP_DETEVAL_MAX_T) return EVREP_EINVAL;
    if (flags & ~(uint32_t)(EVREP_DETEVAL_NATIVE | EVREP_DETEVAL_SKIP_EMPTY)) return EVREP_EINVAL;
    if (bad_ptr(det, 4) || bad_ptr(count, 4) || bad_ptr(iouv_host, 4) || bad_ptr(correct, 1) || bad_ptr(n_labels, 4) || bad_ptr(status, 4))
        return EVREP_EINVAL;
    if (n_t > 0 ? bad_ptr(targets, 4) : misaligned(targets, 4)) return EVREP_EINVAL;
    if (misaligned(detn, 4) || misaligned(tbox, 4) || misaligned(matrix, 8)) return EVREP_EINVAL;
    const bool native = (flags & EVREP_DETEVAL_NATIVE) != 0u;
    if (native ? misaligned(geom, 4) : bad_ptr(geom, 4)) return EVREP_EINVAL;
    if (!native && (img_h < 1 || img_w < 1 || img_h > EVREP_MAX_DIM || img_w > EVREP_MAX_DIM)) return EVREP_EINVAL;
    if (matrix && (nc < 1 || nc > EVREP_NMS_MAX_CLASSES || !(conf == conf) || !(iou_thres == iou_thres))) return EVREP_EINVAL;
    DetevalArgs a;
    memset(&a, 0, sizeof(a));
    for (int32_t i = 0; i < T; ++i) {
        if (!(iouv_host[i] == iouv_host[i])) return EVREP_EINVAL;   // NaN
        a.iouv[i] = iouv_host[i];
    }
    a.det = det; a.count = count; a.targets = targets; a.geom = geom;
    a.matrix = reinterpret_cast<unsigned long long *>(matrix);
    a.correct = correct; a.detn = detn; a.tbox = tbox; a.n_labels = n_labels; a.status = status;
    a.n_t = n_t;
    a.img_h = (float)img_h; a.img_w = (float)img_w; a.conf = conf; a.iou_thres = iou_thres;
    a.B = B; a.max_det = max_det; a.T = T; a.nc = matrix ? nc : 0;
    a.native = native ? 1 : 0;
    a.skip_empty = (flags & EVREP_DETEVAL_SKIP_EMPTY) ? 1 : 0;
    k_det_match<<<(unsigned)B, kDistThreads, 0, as_stream(stream_)>>>(a);
    LAUNCH_CHECK("k_det_match");
    return EVREP_OK;
}

static inline bool ap_shape_ok(int64_t n, int32_t T, int32_t nc) {
    return n >= 0 && n < ((int64_t)1 << 31) && T >= 1 && T <= EVREP_DETEVAL_MAX_T && nc >= 1 && nc <= EVREP_NMS_MAX_CLASSES;
}
static inline int64_t ap_sort_tiles(int64_t n) { return (n + kApSortTile - 1) / kApSortTile; }
static inline int64_t ap_scan_tiles(int64_t n) { return (n + kApScanTile - 1) / kApScanTile; }

// the workspace of evrep_det_ap: the two (key, row) buffers of the sort, its (digit, tile) table, the class counts and
// starts, the sorted confidences, the counts and running maxima per (row, threshold), and the scan tiles' words
static size_t ap_layout(void *ws, int64_t n, int32_t T, int32_t nc, ApArgs *a) {
    Carver c(ws);
    const size_t rows = (size_t)n, st = (size_t)ap_scan_tiles(n);
    unsigned long long *key_a = c.take<unsigned long long>(rows * 8), *key_b = c.take<unsigned long long>(rows * 8);
    uint32_t *idx_a = c.take<uint32_t>(rows * 4), *idx_b = c.take<uint32_t>(rows * 4);
    uint32_t *hist = c.take<uint32_t>(256 * (size_t)ap_sort_tiles(n) * 4);
    uint32_t *cnt_p = c.take<uint32_t>(((size_t)nc + 1) * 4), *cnt_l = c.take<uint32_t>(((size_t)nc + 1) * 4);
    uint32_t *seg = c.take<uint32_t>(((size_t)nc + 2) * 4);
    float *sconf = c.take<float>(rows * 4);
    uint32_t *cum = c.take<uint32_t>(rows * T * 4);
    double *mpre = c.take<double>(rows * T * 8);
    uint32_t *tsum = c.take<uint32_t>(st * T * 4);
    double *thead = c.take<double>(st * T * 8), *tcarry = c.take<double>(st * T * 8);
    uint32_t *tcls_head = c.take<uint32_t>(st * 4), *tcls_tail = c.take<uint32_t>(st * 4);
    if (a) {
        a->key_a = key_a; a->key_b = key_b; a->idx_a = idx_a; a->idx_b = idx_b; a->hist = hist; a->cnt_p = cnt_p; a->cnt_l = cnt_l;
        a->seg = seg; a->sconf = sconf; a->cum = cum; a->mpre = mpre; a->tsum = tsum; a->thead = thead; a->tcarry = tcarry;
        a->tcls_head = tcls_head; a->tcls_tail = tcls_tail;
    }
    return c.off;
}

size_t evrep_det_ap_workspace_bytes(int64_t n, int32_t T, int32_t nc) {
    return ap_shape_ok(n, T, nc) ? ap_layout(nullptr, n, T, nc, nullptr) : 0;
}

int evrep_det_ap_gather(const uint8_t *correct, const float *conf_cls, const int32_t *count, int32_t B, int32_t max_det, int32_t T,
                        const float *targets, int64_t n_t, uint8_t *tp, float *conf, float *pred_cls, int64_t cap_n,
                        float *target_cls, int64_t cap_m, int64_t *cursor, void *stream_) {
    if (B < 1 || B > 65535 || max_det < 1 || max_det > EVREP_NMS_MAX_DET || T < 1 || T > EVREP_DETEVAL_MAX_T) return EVREP_EINVAL;
    if (n_t < 0 || n_t > EVREP_DETEVAL_MAX_TARGETS || cap_m < 0 || cap_m >= ((int64_t)1 << 31)) return EVREP_EINVAL;
    if (cap_n < (int64_t)B * max_det || cap_n >= ((int64_t)1 << 31)) return EVREP_EINVAL;
    if (bad_ptr(correct, 1) || bad_ptr(conf_cls, 4) || bad_ptr(count, 4) || bad_ptr(cursor, 8)) return EVREP_EINVAL;
    if (bad_ptr(tp, 1) || bad_ptr(conf, 4) || bad_ptr(pred_cls, 4)) return EVREP_EINVAL;
    if (n_t > 0 ? bad_ptr(targets, 4) : misaligned(targets, 4)) return EVREP_EINVAL;
    if (n_t > 0 && cap_m > 0 ? bad_ptr(target_cls, 4) : misaligned(target_cls, 4)) return EVREP_EINVAL;
    ApGatherArgs g;
    g.correct = correct; g.conf_cls = conf_cls; g.count = count; g.targets = targets; g.tp = tp; g.conf = conf; g.pcls = pred_cls;
    g.tcls = target_cls; g.cursor = cursor; g.n_t = n_t; g.cap_n = cap_n; g.cap_m = target_cls ? cap_m : 0;
    g.B = B; g.max_det = max_det; g.T = T;
    hipStream_t stream = as_stream(stream_);
    k_ap_gather_rows<<<(unsigned)B, kThreads, 0, stream>>>(g);
    LAUNCH_CHECK("k_ap_gather_rows");
    k_ap_gather_finish<<<1, kDistThreads, 0, stream>>>(g);
    LAUNCH_CHECK("k_ap_gather_finish");
    return EVREP_OK;
}

int evrep_det_ap(const uint8_t *tp, const float *conf, const float *pred_cls, const float *target_cls, int64_t n, int64_t m,
                 int32_t T, int32_t nc, const int64_t *counts_dev, const double *tables, double *p, double *r, double *f1,
                 double *ap, int64_t *n_labels, int64_t *n_pred, uint32_t *any_correct, uint32_t *status, void *workspace,
                 size_t workspace_bytes, void *stream_) {
    if (!ap_shape_ok(n, T, nc) || m < 0 || m >= ((int64_t)1 << 31)) return EVREP_EINVAL;
    if (n > 0 ? (bad_ptr(tp, 1) || bad_ptr(conf, 4) || bad_ptr(pred_cls, 4)) : (misaligned(conf, 4) || misaligned(pred_cls, 4)))
        return EVREP_EINVAL;
    if (m > 0 ? bad_ptr(target_cls, 4) : misaligned(target_cls, 4)) return EVREP_EINVAL;
    if (misaligned(counts_dev, 8) || bad_ptr(tables, 8)) return EVREP_EINVAL;
    if (bad_ptr(p, 8) || bad_ptr(r, 8) || bad_ptr(f1, 8) || bad_ptr(ap, 8) || bad_ptr(n_labels, 8) || bad_ptr(n_pred, 8)) return EVREP_EINVAL;
    if (bad_ptr(any_correct, 4) || bad_ptr(status, 4) || bad_ptr(workspace, 256)) return EVREP_EINVAL;
    if (workspace_bytes < ap_layout(nullptr, n, T, nc, nullptr)) return EVREP_EWORKSPACE;
    ApArgs a;
    memset(&a, 0, sizeof(a));
    a.tp = tp; a.conf = conf; a.pcls = pred_cls; a.tcls = target_cls; a.counts_dev = counts_dev; a.tables = tables;
    a.p = p; a.r = r; a.f1 = f1; a.ap = ap; a.n_labels = n_labels; a.n_pred = n_pred; a.any_correct = any_correct; a.status = status;
    a.n = n; a.m = m; a.T = T; a.nc = nc;
    ap_layout(workspace, n, T, nc, &a);
    hipStream_t stream = as_stream(stream_);
    const size_t curve = (size_t)nc * kApPx * 8;
    const struct { void *at; size_t bytes; const char *what; } zero[] = {
        {p, curve, "hipMemsetAsync(p)"}, {r, curve, "hipMemsetAsync(r)"}, {f1, curve, "hipMemsetAsync(f1)"},
        {ap, (size_t)nc * T * 8, "hipMemsetAsync(ap)"}, {any_correct, 4, "hipMemsetAsync(any_correct)"}, {status, 4, "hipMemsetAsync(status)"},
        {a.cnt_p, ((size_t)nc + 1) * 4, "hipMemsetAsync(cnt_p)"}, {a.cnt_l, ((size_t)nc + 1) * 4, "hipMemsetAsync(cnt_l)"}};
    for (const auto &z : zero) {
        const int rc = hip_check(hipMemsetAsync(z.at, 0, z.bytes, stream), z.what);
        if (rc != EVREP_OK) return rc;
    }
    const auto spread = [](int64_t items) {                             // workgroups of a grid-stride launch
        const int64_t need = (items + kThreads - 1) / kThreads;
        return (unsigned)(need < 1024 ? need : 1024);
    };
    if (n > 0) {
        k_ap_keys<<<spread(n), kThreads, 0, stream>>>(a);
        LAUNCH_CHECK("k_ap_keys");
    }
    if (m > 0) {
        k_ap_targets<<<spread(m), kThreads, 0, stream>>>(a);
        LAUNCH_CHECK("k_ap_targets");
    }
    k_ap_segments<<<1, kDistThreads, 0, stream>>>(a);
    LAUNCH_CHECK("k_ap_segments");
    if (n == 0) return EVREP_OK;
    ApSortArgs s;
    s.hist = a.hist; s.tiles = (int32_t)ap_sort_tiles(n);
    const int passes = 4 + (nc + 1 <= 256 ? 1 : 2);                     // the 32 bits of the confidence, then the class's
    for (int pass = 0; pass < passes; ++pass) {
        const bool even = (pass & 1) == 0;
        s.key_in = even ? a.key_a : a.key_b; s.idx_in = even ? a.idx_a : a.idx_b;
        s.key_out = even ? a.key_b : a.key_a; s.idx_out = even ? a.idx_b : a.idx_a;
        s.shift = 8 * pass;
        k_ap_radix_count<<<(unsigned)s.tiles, kThreads, 0, stream>>>(a, s);
        LAUNCH_CHECK("k_ap_radix_count");
        k_ap_radix_scan<<<1, kDistThreads, 0, stream>>>(s);
        LAUNCH_CHECK("k_ap_radix_scan");
        k_ap_radix_scatter<<<(unsigned)s.tiles, kThreads, 0, stream>>>(a, s);
        LAUNCH_CHECK("k_ap_radix_scatter");
    }
    const unsigned long long *key = (passes & 1) ? a.key_b : a.key_a;
    const uint32_t *idx = (passes & 1) ? a.idx_b : a.idx_a;
    const unsigned wave_tiles = (unsigned)((ap_scan_tiles(n) + kWaves - 1) / kWaves);
    k_ap_cum<false><<<wave_tiles, kThreads, 0, stream>>>(a, idx);
    LAUNCH_CHECK("k_ap_cum<sums>");
    k_ap_cum_scan<<<1, kWave, 0, stream>>>(a);
    LAUNCH_CHECK("k_ap_cum_scan");
    if (m == 0) return EVREP_OK;                                        // no class has a label: every curve stays zero
    k_ap_cum<true><<<wave_tiles, kThreads, 0, stream>>>(a, idx);
    LAUNCH_CHECK("k_ap_cum<write>");
    k_ap_sorted_conf<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, stream>>>(a, idx);
    LAUNCH_CHECK("k_ap_sorted_conf");
    k_ap_max<false><<<wave_tiles, kThreads, 0, stream>>>(a, key);
    LAUNCH_CHECK("k_ap_max<heads>");
    k_ap_max_carry<<<1, kWave, 0, stream>>>(a);
    LAUNCH_CHECK("k_ap_max_carry");
    k_ap_max<true><<<wave_tiles, kThreads, 0, stream>>>(a, key);
    LAUNCH_CHECK("k_ap_max<write>");
    k_ap_curves<<<dim3((kApPx + kThreads - 1) / kThreads, (unsigned)nc), kThreads, 0, stream>>>(a);
    LAUNCH_CHECK("k_ap_curves");
    k_ap_area<<<(unsigned)(((int64_t)nc * T + kWaves - 1) / kWaves), kThreads, 0, stream>>>(a);
    LAUNCH_CHECK("k_ap_area");
    return EVREP_OK;
}

int evrep_det_targets_pad(const float *targets, int64_t n_t, int32_t B, int32_t M, float width, float height, double *gt,
                          int32_t *n_labels, uint32_t *status, void *stream_) {
    if (B < 1 || B > 65535 || M < 0 || M > EVREP_TAL_MAX_LABELS || n_t < 0 || n_t > EVREP_DETEVAL_MAX_TARGETS) return EVREP_EINVAL;
    if (!(width - width == 0.0f) || !(height - height == 0.0f)) return EVREP_EINVAL;   // NaN, inf
    if (n_t > 0 ? bad_ptr(targets, 4) : misaligned(targets, 4)) return EVREP_EINVAL;
    if (M > 0 ? bad_ptr(gt, 8) : misaligned(gt, 8)) return EVREP_EINVAL;
    if (bad_ptr(n_labels, 4) || bad_ptr(status, 4)) return EVREP_EINVAL;
    TalPadArgs a;
    a.targets = targets; a.gt = gt; a.n_labels = n_labels; a.status = status;
    a.n_t = n_t; a.W = (double)width; a.H = (double)height; a.B = B; a.M = M;
    k_det_targets_pad<<<(unsigned)B, kDistThreads, 0, as_stream(stream_)>>>(a);
    LAUNCH_CHECK("k_det_targets_pad");
    return EVREP_OK;
}

static inline bool tal_shape_ok(int32_t B, int32_t M, int32_t A) {
    return B >= 1 && B <= 65535 && M >= 0 && M <= EVREP_TAL_MAX_LABELS && A >= 1 && A <= EVREP_TAL_MAX_ANCHORS;
}

// workgroups per image of a launch that could use `need` of them: B * G about 2048, at least one
static inline unsigned groups_per_image(size_t need, int32_t B) {
    const size_t cap = (2048 + (size_t)B - 1) / (size_t)B;
    return (unsigned)(need < 1 ? 1 : (need < cap ? need : cap));
}
// the same for a grid-stride launch over `items` elements of an image, a lane each
static inline unsigned groups_per_image_of(size_t items, int32_t B) {
    return groups_per_image((items + kThreads - 1) / kThreads, B);
}

// what both assigners check alike of the label rows, the five outputs and the scratch: non-null (gt but for M == 0) and aligned
static inline bool assign_ptrs_ok(const double *gt, int32_t M, const int64_t *labels, const void *boxes, uintptr_t elem_boxes,
                                  const void *scores, uintptr_t elem_scores, const uint8_t *fg, const uint32_t *status,
                                  const void *scratch) {
    if (M > 0 ? bad_ptr(gt, 8) : misaligned(gt, 8)) return false;
    if (bad_ptr(labels, 8) || bad_ptr(boxes, elem_boxes) || bad_ptr(scores, elem_scores) || bad_ptr(fg, 1)) return false;
    return !(bad_ptr(status, 4) || bad_ptr(scratch, 256));
}

// the scratch of evrep_tal_assign: the claim arrays; per (image, row) the two maxima
static size_t tal_layout(void *scratch, int32_t B, int32_t M, int32_t A, TalArgs *t) {
    Carver c(scratch);
    const size_t bm = (size_t)B * (size_t)M;
    claim_layout(c, B, A, t);
    unsigned long long *pos_al = c.take<unsigned long long>(bm * 8);
    unsigned long long *pos_ov = c.take<unsigned long long>(bm * 8);
    if (t) {
        t->pos_al = pos_al; t->pos_ov = pos_ov;
    }
    return c.off;
}

size_t evrep_tal_workspace_bytes(int32_t B, int32_t M, int32_t A) {
    return tal_shape_ok(B, M, A) ? tal_layout(nullptr, B, M, A, nullptr) : 0;
}

int evrep_tal_assign(const float *pd_scores, const float *pd_bboxes, const float *anc_points, const double *gt, int32_t B,
                     int32_t M, int32_t A, int32_t nc, int32_t topk, int32_t alpha, int32_t beta, uint32_t flags,
                     int64_t *target_labels, void *target_bboxes, void *target_scores, uint8_t *fg, uint32_t *status,
                     void *scratch, void *stream_) {
    if (!tal_shape_ok(B, M, A) || nc < 1 || nc > EVREP_TAL_MAX_CLASSES || (int64_t)A * nc > INT32_MAX) return EVREP_EINVAL;
    if (topk < 1 || topk > EVREP_TAL_MAX_TOPK || alpha < 0 || alpha > EVREP_TAL_MAX_POWER || beta < 0 || beta > EVREP_TAL_MAX_POWER)
        return EVREP_EINVAL;
    if (flags & ~(uint32_t)EVREP_TAL_F32_OUT) return EVREP_EINVAL;
    const uintptr_t elem = (flags & EVREP_TAL_F32_OUT) ? 4 : 8;
    if (bad_ptr(pd_scores, 4) || bad_ptr(pd_bboxes, 4) || bad_ptr(anc_points, 4)) return EVREP_EINVAL;
    if (!assign_ptrs_ok(gt, M, target_labels, target_bboxes, elem, target_scores, elem, fg, status, scratch)) return EVREP_EINVAL;
    TalArgs t;
    memset(&t, 0, sizeof(t));
    t.pd_scores = pd_scores; t.pd_bboxes = pd_bboxes; t.anc = anc_points; t.gt = gt;
    t.labels = target_labels; t.boxes = target_bboxes; t.scores = target_scores; t.fg = fg; t.status = status;
    t.B = B; t.M = M; t.A = A; t.nc = nc; t.topk = topk; t.alpha = alpha; t.beta = beta;
    t.f32_out = (flags & EVREP_TAL_F32_OUT) ? 1 : 0;
    tal_layout(scratch, B, M, A, &t);
    hipStream_t stream = as_stream(stream_);
    int rc = hip_check(hipMemsetAsync(status, 0, (size_t)B * 4u, stream), "hipMemsetAsync(status)");
    if (rc != EVREP_OK) return rc;
    if (M > 0) {
        k_tal_prepare<<<dim3(groups_per_image_of((size_t)A * nc, B), (unsigned)B), kThreads, 0, stream>>>(t);
        LAUNCH_CHECK("k_tal_prepare");
        k_tal_select<<<dim3((unsigned)M, (unsigned)B), kTalSelectThreads, 0, stream>>>(t);
        LAUNCH_CHECK("k_tal_select");
    }
    k_tal_resolve<<<dim3((unsigned)((A + kThreads - 1) / kThreads), (unsigned)B), kThreads, 0, stream>>>(t);
    LAUNCH_CHECK("k_tal_resolve");
    k_tal_scores<<<dim3(groups_per_image_of((size_t)A * nc, B), (unsigned)B), kThreads, 0, stream>>>(t);
    LAUNCH_CHECK("k_tal_scores");
    return EVREP_OK;
}

// the scratch of evrep_atss_assign: the claim arrays
static size_t atss_layout(void *scratch, int32_t B, int32_t A, AtssArgs *t) {
    Carver c(scratch);
    claim_layout(c, B, A, t);
    return c.off;
}

size_t evrep_atss_workspace_bytes(int32_t B, int32_t M, int32_t A) {
    return tal_shape_ok(B, M, A) ? atss_layout(nullptr, B, A, nullptr) : 0;
}

int evrep_atss_assign(const float *anchors, const int32_t *level_counts, int32_t n_levels, const double *gt, const float *pd_bboxes,
                      int32_t B, int32_t M, int32_t A, int32_t nc, int32_t topk, uint32_t flags, int64_t *target_labels,
                      void *target_bboxes, void *target_scores, uint8_t *fg, uint32_t *status, void *scratch, void *stream_) {
    if (!tal_shape_ok(B, M, A) || nc < 1 || nc > EVREP_TAL_MAX_CLASSES || (int64_t)A * nc > INT32_MAX) return EVREP_EINVAL;
    if (topk < 1 || topk > EVREP_ATSS_MAX_TOPK || n_levels < 1 || n_levels > EVREP_ATSS_MAX_LEVELS || n_levels * topk > EVREP_ATSS_MAX_CANDIDATES || !level_counts)
        return EVREP_EINVAL;
    if (flags & ~(uint32_t)(EVREP_ATSS_F32_BOXES | EVREP_ATSS_F32_SCORES)) return EVREP_EINVAL;
    AtssArgs t;
    memset(&t, 0, sizeof(t));
    int64_t total = 0;
    for (int32_t l = 0; l < n_levels; ++l) {
        if (level_counts[l] < topk || level_counts[l] > A) return EVREP_EINVAL;
        t.lvl_start[l] = (int32_t)total;                                // <= A: the sum is held to A below
        t.lvl_n[l] = level_counts[l];
        total += level_counts[l];
        if (total > A) return EVREP_EINVAL;
    }
    if (total != A) return EVREP_EINVAL;
    const uintptr_t elem_b = (flags & EVREP_ATSS_F32_BOXES) ? 4 : 8, elem_s = (flags & EVREP_ATSS_F32_SCORES) ? 4 : 8;
    if (bad_ptr(anchors, 4) || misaligned(pd_bboxes, 4)) return EVREP_EINVAL;
    if (!assign_ptrs_ok(gt, M, target_labels, target_bboxes, elem_b, target_scores, elem_s, fg, status, scratch)) return EVREP_EINVAL;
    t.anchors = anchors; t.pd_bboxes = pd_bboxes; t.gt = gt;
    t.labels = target_labels; t.boxes = target_bboxes; t.scores = target_scores; t.fg = fg; t.status = status;
    t.B = B; t.M = M; t.A = A; t.nc = nc; t.topk = topk; t.n_levels = n_levels;
    t.f32_boxes = (flags & EVREP_ATSS_F32_BOXES) ? 1 : 0;
    t.f32_scores = (flags & EVREP_ATSS_F32_SCORES) ? 1 : 0;
    atss_layout(scratch, B, A, &t);
    hipStream_t stream = as_stream(stream_);
    int rc = hip_check(hipMemsetAsync(status, 0, (size_t)B * 4u, stream), "hipMemsetAsync(status)");
    if (rc != EVREP_OK) return rc;
    if (M > 0) {
        k_atss_prepare<<<dim3(groups_per_image_of((size_t)A * 4u, B), (unsigned)B), kThreads, 0, stream>>>(t);
        LAUNCH_CHECK("k_atss_prepare");
        k_atss_select<<<dim3((unsigned)M, (unsigned)B), kAtssThreads, 0, stream>>>(t);
        LAUNCH_CHECK("k_atss_select");
    }
    k_atss_resolve<<<dim3((unsigned)((A + kThreads - 1) / kThreads), (unsigned)B), kThreads, 0, stream>>>(t);
    LAUNCH_CHECK("k_atss_resolve");
    k_atss_scores<<<dim3(groups_per_image_of((size_t)A * nc, B), (unsigned)B), kThreads, 0, stream>>>(t);
    LAUNCH_CHECK("k_atss_scores");
    return EVREP_OK;
}

static inline bool detloss_shape_ok(int32_t B, int32_t A, int32_t nc) {
    return B >= 1 && B <= 65535 && A >= 1 && A <= EVREP_TAL_MAX_ANCHORS && nc >= 1 && nc <= EVREP_TAL_MAX_CLASSES && (int64_t)A * nc <= INT32_MAX;
}

// the grids of evrep_detloss: slices of tss, workgroups per image of the class term, workgroups per image of the box terms
static inline uint32_t detloss_n_tss(int32_t B, int32_t A) {
    const size_t chunks = ((size_t)B * (size_t)A + kThreads - 1) / kThreads;
    return (uint32_t)(chunks < (size_t)kDetlossSlices ? chunks : (size_t)kDetlossSlices);
}
static inline uint32_t detloss_gc(int32_t B, int32_t A, int32_t nc) { return groups_per_image_of((size_t)A * (size_t)nc, B); }
static inline uint32_t detloss_ga(int32_t A) { return (uint32_t)((A + kThreads - 1) / kThreads); }
// workgroups per image of the distilled class term: a tile of whole rows each, dealt round robin
static inline uint32_t detdistill_gd(int32_t B, int32_t A, int32_t nc) {
    const size_t rt = (size_t)distill_tile_rows(nc);
    return groups_per_image(((size_t)A + rt - 1) / rt, B);
}

// the scratch of evrep_detloss: the rows' sums per (image, anchor), then the partial sums of the four launches.  That of
// evrep_detloss_distill (`distill`) has three arrays per slice of the rows launch, not one, two per workgroup of its own class
// launch, and four per workgroup of the box launch, not three.
static size_t detloss_layout(void *scratch, int32_t B, int32_t A, int32_t nc, bool distill, DetlossArgs *t) {
    Carver c(scratch);
    const size_t n_tss = detloss_n_tss(B, A), n_box = (size_t)B * detloss_ga(A);
    const size_t n_cls = (size_t)B * (distill ? detdistill_gd(B, A, nc) : detloss_gc(B, A, nc));
    double *w = c.take<double>((size_t)B * (size_t)A * 8);
    double *tss_part = c.take<double>(n_tss * 8);
    double *wfg_part = distill ? c.take<double>(n_tss * 8) : nullptr;
    double *nfg_part = distill ? c.take<double>(n_tss * 8) : nullptr;
    double *cls_part = c.take<double>(n_cls * 8);
    double *dcls_part = distill ? c.take<double>(n_cls * 8) : nullptr;
    double *iou_part = c.take<double>(n_box * 8);
    double *dfl_part = c.take<double>(n_box * 8);
    double *cnt_part = c.take<double>(n_box * 8);
    double *ddfl_part = distill ? c.take<double>(n_box * 8) : nullptr;
    if (t) {
        t->w = w; t->tss_part = tss_part; t->wfg_part = wfg_part; t->nfg_part = nfg_part; t->cls_part = cls_part; t->dcls_part = dcls_part;
        t->iou_part = iou_part; t->dfl_part = dfl_part; t->cnt_part = cnt_part; t->ddfl_part = ddfl_part;
        t->n_tss = (uint32_t)n_tss; t->n_cls = (uint32_t)n_cls; t->n_box = (uint32_t)n_box;
    }
    return c.off;
}

size_t evrep_detloss_workspace_bytes(int32_t B, int32_t A, int32_t nc) {
    return detloss_shape_ok(B, A, nc) ? detloss_layout(nullptr, B, A, nc, false, nullptr) : 0;
}

size_t evrep_detloss_distill_workspace_bytes(int32_t B, int32_t A, int32_t nc) {
    return detloss_shape_ok(B, A, nc) && nc <= EVREP_DISTILL_MAX_CLASSES ? detloss_layout(nullptr, B, A, nc, true, nullptr) : 0;
}

// R with DFL: 1..32 (the bins tl and tl + 1 of a target lie inside the R + 1 logits); without: 0..32, not read
static inline bool detloss_r_ok(int32_t R, uint32_t flags) {
    return R <= EVREP_DETLOSS_MAX_REG && R >= ((flags & EVREP_DETLOSS_USE_DFL) ? 1 : 0);
}

int evrep_detloss_decode(const float *pred_distri, const float *anc_points, const float *stride, int32_t B, int32_t A, int32_t R,
                         uint32_t flags, float *boxes_s, float *boxes_px, void *stream_) {
    if (B < 1 || B > 65535 || A < 1 || A > EVREP_TAL_MAX_ANCHORS) return EVREP_EINVAL;
    if ((flags & ~(uint32_t)EVREP_DETLOSS_USE_DFL) || !detloss_r_ok(R, flags)) return EVREP_EINVAL;
    if (bad_ptr(pred_distri, 4) || bad_ptr(anc_points, 4) || bad_ptr(stride, 4) || bad_ptr(boxes_s, 4) || bad_ptr(boxes_px, 4))
        return EVREP_EINVAL;
    DetlossArgs t;
    memset(&t, 0, sizeof(t));
    t.z = pred_distri; t.anc = anc_points; t.stride = stride; t.boxes_s = boxes_s; t.boxes_px = boxes_px;
    t.B = B; t.A = A; t.R = R;
    t.use_dfl = (flags & EVREP_DETLOSS_USE_DFL) ? 1 : 0;
    t.K = t.use_dfl ? R + 1 : 1;
    k_detloss_decode<<<dim3((unsigned)((4 * (size_t)A + kThreads - 1) / kThreads), (unsigned)B), kThreads, 0, as_stream(stream_)>>>(t);
    LAUNCH_CHECK("k_detloss_decode");
    return EVREP_OK;
}

// What evrep_detloss and evrep_detloss_distill share: the checks of the shape, the flags and the pointers both take, and *t
// zeroed and filled from them -- all but the teacher's fields and the scratch, which the entry adds.
static int detloss_args(const float *pred_scores, const float *pred_distri, const float *anc_points, const float *stride,
                        const int64_t *target_labels, const void *target_bboxes, const void *target_scores, const uint8_t *fg,
                        int32_t B, int32_t A, int32_t nc, int32_t R, double w_class, double w_iou, double w_dfl, uint32_t flags,
                        double *losses, float *grad_scores, float *grad_distri, uint32_t *status, const void *scratch,
                        DetlossArgs *t) {
    if (!detloss_shape_ok(B, A, nc)) return EVREP_EINVAL;
    if ((flags & ~(uint32_t)(EVREP_DETLOSS_USE_DFL | EVREP_DETLOSS_NO_GRAD | EVREP_DETLOSS_F32_TARGETS)) || !detloss_r_ok(R, flags))
        return EVREP_EINVAL;
    const uintptr_t elem = (flags & EVREP_DETLOSS_F32_TARGETS) ? 4 : 8;
    const bool grad = !(flags & EVREP_DETLOSS_NO_GRAD);
    if (bad_ptr(pred_scores, 4) || bad_ptr(pred_distri, 4) || bad_ptr(anc_points, 4) || bad_ptr(stride, 4)) return EVREP_EINVAL;
    if (bad_ptr(target_labels, 8) || bad_ptr(target_bboxes, elem) || bad_ptr(target_scores, elem) || bad_ptr(fg, 1)) return EVREP_EINVAL;
    if (grad ? (bad_ptr(grad_scores, 4) || bad_ptr(grad_distri, 4)) : (misaligned(grad_scores, 4) || misaligned(grad_distri, 4)))
        return EVREP_EINVAL;
    if (bad_ptr(losses, 8) || bad_ptr(status, 4) || bad_ptr(scratch, 256)) return EVREP_EINVAL;
    memset(t, 0, sizeof(*t));
    t->p = pred_scores; t->z = pred_distri; t->anc = anc_points; t->stride = stride;
    t->labels = target_labels; t->tb = target_bboxes; t->ts = target_scores; t->fg = fg;
    t->losses = losses; t->gs = grad ? grad_scores : nullptr; t->gz = grad ? grad_distri : nullptr; t->status = status;
    t->wc = w_class; t->wi = w_iou; t->wd = w_dfl;
    t->B = B; t->A = A; t->nc = nc; t->R = R;
    t->use_dfl = (flags & EVREP_DETLOSS_USE_DFL) ? 1 : 0;
    t->K = t->use_dfl ? R + 1 : 1;
    t->f32_t = (flags & EVREP_DETLOSS_F32_TARGETS) ? 1 : 0;
    t->grad = grad ? 1 : 0;
    return EVREP_OK;
}

int evrep_detloss(const float *pred_scores, const float *pred_distri, const float *anc_points, const float *stride,
                  const int64_t *target_labels, const void *target_bboxes, const void *target_scores, const uint8_t *fg, int32_t B,
                  int32_t A, int32_t nc, int32_t R, double w_class, double w_iou, double w_dfl, uint32_t flags, double *losses,
                  float *grad_scores, float *grad_distri, uint32_t *status, void *scratch, void *stream_) {
    DetlossArgs t;
    int rc = detloss_args(pred_scores, pred_distri, anc_points, stride, target_labels, target_bboxes, target_scores, fg, B, A, nc, R,
                          w_class, w_iou, w_dfl, flags, losses, grad_scores, grad_distri, status, scratch, &t);
    if (rc != EVREP_OK) return rc;
    detloss_layout(scratch, B, A, nc, false, &t);
    hipStream_t stream = as_stream(stream_);
    rc = hip_check(hipMemsetAsync(status, 0, (size_t)B * 4u, stream), "hipMemsetAsync(status)");
    if (rc != EVREP_OK) return rc;
    k_detloss_rows<false><<<t.n_tss, kThreads, 0, stream>>>(t);
    LAUNCH_CHECK("k_detloss_rows");
    k_detloss_cls<<<dim3(detloss_gc(B, A, nc), (unsigned)B), kThreads, 0, stream>>>(t);
    LAUNCH_CHECK("k_detloss_cls");
    k_detloss_box<false><<<dim3(detloss_ga(A), (unsigned)B), kThreads, 0, stream>>>(t);
    LAUNCH_CHECK("k_detloss_box");
    k_detloss_fold<false><<<1, kThreads, 0, stream>>>(t);
    LAUNCH_CHECK("k_detloss_fold");
    return EVREP_OK;
}

int evrep_detloss_distill(const float *pred_scores, const float *pred_distri, const float *t_pred_scores, const float *t_pred_distri,
                          const float *anc_points, const float *stride, const int64_t *target_labels, const void *target_bboxes,
                          const void *target_scores, const uint8_t *fg, int32_t B, int32_t A, int32_t nc, int32_t R, double w_class,
                          double w_iou, double w_dfl, double temperature, double k_class, double k_dfl, uint32_t flags, double *losses,
                          float *grad_scores, float *grad_distri, uint32_t *status, void *scratch, void *stream_) {
    if (nc > EVREP_DISTILL_MAX_CLASSES) return EVREP_EINVAL;
    if (!(temperature > 0.0) || !(temperature - temperature == 0.0)) return EVREP_EINVAL;   // NaN, inf, <= 0
    if (bad_ptr(t_pred_scores, 4) || bad_ptr(t_pred_distri, 4)) return EVREP_EINVAL;
    DetlossArgs t;
    int rc = detloss_args(pred_scores, pred_distri, anc_points, stride, target_labels, target_bboxes, target_scores, fg, B, A, nc, R,
                          w_class, w_iou, w_dfl, flags, losses, grad_scores, grad_distri, status, scratch, &t);
    if (rc != EVREP_OK) return rc;
    t.tp = t_pred_scores; t.tz = t_pred_distri;
    t.T = temperature; t.k_class = k_class; t.k_dfl = k_dfl;
    detloss_layout(scratch, B, A, nc, true, &t);
    hipStream_t stream = as_stream(stream_);
    rc = hip_check(hipMemsetAsync(status, 0, (size_t)B * 4u, stream), "hipMemsetAsync(status)");
    if (rc != EVREP_OK) return rc;
    k_detloss_rows<true><<<t.n_tss, kThreads, 0, stream>>>(t);
    LAUNCH_CHECK("k_detloss_rows<distill>");
    k_detdistill_cls<<<dim3(detdistill_gd(B, A, nc), (unsigned)B), kThreads, 0, stream>>>(t);
    LAUNCH_CHECK("k_detdistill_cls");
    k_detloss_box<true><<<dim3(detloss_ga(A), (unsigned)B), kThreads, 0, stream>>>(t);
    LAUNCH_CHECK("k_detloss_box<distill>");
    k_detloss_fold<true><<<1, kThreads, 0, stream>>>(t);
    LAUNCH_CHECK("k_detloss_fold<distill>");
    return EVREP_OK;
}

// the levels of evrep_detloss_cwd: counts, offsets and scales; false for a refused table
// (the two level structs differ in the pointee types of s and t only: the float32 entry's table is read as the typed one)
static_assert(sizeof(evrep_cwd_level) == sizeof(evrep_cwd_level_typed) && offsetof(evrep_cwd_level, grad_s) == offsetof(evrep_cwd_level_typed, grad_s) &&
              offsetof(evrep_cwd_level, n) == offsetof(evrep_cwd_level_typed, n), "one layout");

// the bytes of a map element of dtype code dt; 0 for an unknown code
static inline uintptr_t dt_size(int32_t dt) { return dt == EVREP_DT_F32 ? 4u : (dt == EVREP_DT_F16 || dt == EVREP_DT_BF16) ? 2u : 0u; }

static bool cwd_levels(const evrep_cwd_level_typed *lv, int32_t L, double tau, bool grad, int32_t sdt, int32_t tdt, CwdArgs *t,
                       int64_t *rows_out) {
    if (L < 1 || L > EVREP_CWD_MAX_LEVELS || bad_ptr(lv, 8) || !dt_size(sdt) || !dt_size(tdt)) return false;
    int64_t rows = 0;
    for (int32_t l = 0; l < L; ++l) {
        const evrep_cwd_level_typed &v = lv[l];
        if (v.n < 1 || v.c < 1 || v.h < 1 || v.w < 1) return false;
        if ((int64_t)v.n * v.c > EVREP_TAL_MAX_ANCHORS || (int64_t)v.h * v.w > EVREP_TAL_MAX_ANCHORS) return false;
        if (t) {
            if (bad_ptr(v.s, dt_size(sdt)) || bad_ptr(v.t, dt_size(tdt)) || (grad ? bad_ptr(v.grad_s, 4) : misaligned(v.grad_s, 4)))
                return false;
            const double nc = (double)((int64_t)v.n * v.c);
            t->s[l] = v.s; t->t[l] = v.t; t->g[l] = grad ? v.grad_s : nullptr;
            t->hw[l] = v.h * v.w; t->rows[l] = v.n * v.c; t->row0[l] = (int32_t)rows;
            t->gscale[l] = tau / nc;
            t->lscale[l] = (tau * tau) / nc;
        }
        rows += (int64_t)v.n * v.c;
    }
    if (rows > EVREP_TAL_MAX_ANCHORS) return false;
    *rows_out = rows;
    return true;
}

size_t evrep_detloss_cwd_typed_workspace_bytes(const evrep_cwd_level_typed *levels_host, int32_t L) {
    int64_t rows = 0;
    if (!cwd_levels(levels_host, L, 1.0, false, EVREP_DT_F32, EVREP_DT_F32, nullptr, &rows)) return 0;
    Carver c(nullptr);
    c.take<double>((size_t)rows * 8);
    return c.off;
}

size_t evrep_detloss_cwd_workspace_bytes(const evrep_cwd_level *levels_host, int32_t L) {
    return evrep_detloss_cwd_typed_workspace_bytes(reinterpret_cast<const evrep_cwd_level_typed *>(levels_host), L);
}

int evrep_detloss_cwd_typed(const evrep_cwd_level_typed *levels_host, int32_t L, double tau, uint32_t flags, int32_t s_dtype,
                            int32_t t_dtype, double *out, void *scratch, void *stream_) {
    if (flags & ~(uint32_t)EVREP_DETLOSS_NO_GRAD) return EVREP_EINVAL;
    if (!(tau > 0.0) || !(tau - tau == 0.0)) return EVREP_EINVAL;
    if (bad_ptr(out, 8) || bad_ptr(scratch, 256)) return EVREP_EINVAL;
    CwdArgs t;
    memset(&t, 0, sizeof(t));
    int64_t rows = 0;
    if (!cwd_levels(levels_host, L, tau, !(flags & EVREP_DETLOSS_NO_GRAD), s_dtype, t_dtype, &t, &rows)) return EVREP_EINVAL;
    Carver c(scratch);
    t.part = c.take<double>((size_t)rows * 8);
    t.out = out; t.tau = tau; t.L = L; t.sdt = s_dtype; t.tdt = t_dtype;
    hipStream_t stream = as_stream(stream_);
    if (s_dtype == EVREP_DT_F32 && t_dtype == EVREP_DT_F32) k_detdistill_cw<false><<<(unsigned)rows, kThreads, 0, stream>>>(t);
    else k_detdistill_cw<true><<<(unsigned)rows, kThreads, 0, stream>>>(t);
    LAUNCH_CHECK("k_detdistill_cw");
    k_detdistill_cw_fold<<<1, kThreads, 0, stream>>>(t);
    LAUNCH_CHECK("k_detdistill_cw_fold");
    return EVREP_OK;
}

int evrep_detloss_cwd(const evrep_cwd_level *levels_host, int32_t L, double tau, uint32_t flags, double *out, void *scratch,
                      void *stream_) {
    return evrep_detloss_cwd_typed(reinterpret_cast<const evrep_cwd_level_typed *>(levels_host), L, tau, flags, EVREP_DT_F32,
                                   EVREP_DT_F32, out, scratch, stream_);
}

// widen (dir 0: src 16-bit, dst float32) or round (dir 1: src float32, dst 16-bit) n elements on the HOST by the functions the
// kernels use
int evrep_cast16_host(const void *src, void *dst, int64_t n, int32_t dtype, int32_t dir) {
    if ((dtype != EVREP_DT_F16 && dtype != EVREP_DT_BF16) || (dir != 0 && dir != 1) || n < 0) return EVREP_EINVAL;
    if (n > 0 && (bad_ptr(src, dir ? 4 : 2) || bad_ptr(dst, dir ? 2 : 4))) return EVREP_EINVAL;
    for (int64_t i = 0; i < n; ++i) {
        if (dir) static_cast<uint16_t *>(dst)[i] = round16(static_cast<const float *>(src)[i], dtype);
        else static_cast<float *>(dst)[i] = widen16(static_cast<const uint16_t *>(src)[i], dtype);
    }
    return EVREP_OK;
}

// the shape checks the three evrep_dethead_* entries share; fills the counts of the level table
static inline bool dethead_shape_ok(int32_t L, int32_t B, int32_t nc, int32_t R, uint32_t flags) {
    if (L < 1 || L > EVREP_DETHEAD_MAX_LEVELS || B < 1 || B > 65535 || nc < 1 || nc > EVREP_TAL_MAX_CLASSES) return false;
    if (flags & ~(uint32_t)EVREP_DETHEAD_USE_DFL) return false;
    return R >= ((flags & EVREP_DETHEAD_USE_DFL) ? 1 : 0) && R <= EVREP_DETLOSS_MAX_REG;
}

static inline bool dethead_level(DetheadArgs &t, int32_t l, int32_t h, int32_t w, int64_t &total, int64_t &tiles) {
    if (h < 1 || w < 1 || (int64_t)h * w > EVREP_TAL_MAX_ANCHORS) return false;
    t.n[l] = h * w; t.w[l] = w; t.off[l] = (int32_t)total; t.tile0[l] = (int32_t)tiles;
    total += t.n[l];
    tiles += (t.n[l] + kDetheadTile - 1) / kDetheadTile;
    return total <= EVREP_TAL_MAX_ANCHORS;
}

static_assert(sizeof(evrep_dethead_level) == sizeof(evrep_dethead_level_typed) && offsetof(evrep_dethead_level, h) == offsetof(evrep_dethead_level_typed, h) &&
              offsetof(evrep_dethead_level, stride) == offsetof(evrep_dethead_level_typed, stride) &&
              sizeof(evrep_dethead_grad_level) == sizeof(evrep_dethead_grad_level_typed) &&
              offsetof(evrep_dethead_grad_level, h) == offsetof(evrep_dethead_grad_level_typed, h), "one layout");

// a launch of the kernel template K<dtype> (the dtype was checked)
#define DETHEAD_LAUNCH(K, dtype, grid, stream, t)                                                              \
    do {                                                                                                       \
        if ((dtype) == EVREP_DT_F32) K<EVREP_DT_F32><<<grid, kThreads, 0, stream>>>(t);                         \
        else if ((dtype) == EVREP_DT_F16) K<EVREP_DT_F16><<<grid, kThreads, 0, stream>>>(t);                    \
        else K<EVREP_DT_BF16><<<grid, kThreads, 0, stream>>>(t);                                               \
    } while (0)

static int dethead_forward(const evrep_dethead_level_typed *lv, int32_t L, int32_t B, int32_t nc, int32_t R, uint32_t flags,
                           int32_t dtype, float *pred, float *scores, float *distri, bool train, void *stream_) {
    const uintptr_t elem = dt_size(dtype);
    if (!dethead_shape_ok(L, B, nc, R, flags) || bad_ptr(lv, 8) || !elem) return EVREP_EINVAL;
    if (train ? (bad_ptr(scores, 4) || bad_ptr(distri, 4)) : bad_ptr(pred, 4)) return EVREP_EINVAL;
    DetheadArgs t;
    memset(&t, 0, sizeof(t));
    int64_t total = 0, tiles = 0;
    for (int32_t l = 0; l < L; ++l) {
        if (!dethead_level(t, l, lv[l].h, lv[l].w, total, tiles)) return EVREP_EINVAL;
        if (bad_ptr(lv[l].cls, elem) || bad_ptr(lv[l].reg, elem)) return EVREP_EINVAL;
        if (!(lv[l].stride > 0.0f) || !(lv[l].stride - lv[l].stride == 0.0f)) return EVREP_EINVAL;   // NaN, inf, <= 0
        t.cls[l] = lv[l].cls; t.reg[l] = lv[l].reg; t.stride[l] = lv[l].stride;
    }
    t.pred = pred; t.scores = scores; t.distri = distri;
    t.L = L; t.N = (int32_t)total; t.nc = nc;
    t.use_dfl = (flags & EVREP_DETHEAD_USE_DFL) ? 1 : 0;
    t.K = t.use_dfl ? R + 1 : 1;
    const dim3 grid((unsigned)tiles, (unsigned)B);
    if (train) {
        DETHEAD_LAUNCH(k_dethead_train, dtype, grid, as_stream(stream_), t);
        LAUNCH_CHECK("k_dethead_train");
    } else {
        DETHEAD_LAUNCH(k_dethead_predict, dtype, grid, as_stream(stream_), t);
        LAUNCH_CHECK("k_dethead_predict");
    }
    return EVREP_OK;
}

int evrep_dethead_predict(const evrep_dethead_level *levels_host, int32_t L, int32_t B, int32_t nc, int32_t R, uint32_t flags,
                          float *pred, void *stream_) {
    return dethead_forward(reinterpret_cast<const evrep_dethead_level_typed *>(levels_host), L, B, nc, R, flags, EVREP_DT_F32, pred,
                           nullptr, nullptr, false, stream_);
}

int evrep_dethead_train(const evrep_dethead_level *levels_host, int32_t L, int32_t B, int32_t nc, int32_t R, uint32_t flags,
                        float *pred_scores, float *pred_distri, void *stream_) {
    return dethead_forward(reinterpret_cast<const evrep_dethead_level_typed *>(levels_host), L, B, nc, R, flags, EVREP_DT_F32, nullptr,
                           pred_scores, pred_distri, true, stream_);
}

int evrep_dethead_predict_typed(const evrep_dethead_level_typed *levels_host, int32_t L, int32_t B, int32_t nc, int32_t R,
                                uint32_t flags, int32_t dtype, float *pred, void *stream_) {
    return dethead_forward(levels_host, L, B, nc, R, flags, dtype, pred, nullptr, nullptr, false, stream_);
}

int evrep_dethead_train_typed(const evrep_dethead_level_typed *levels_host, int32_t L, int32_t B, int32_t nc, int32_t R,
                              uint32_t flags, int32_t dtype, float *pred_scores, float *pred_distri, void *stream_) {
    return dethead_forward(levels_host, L, B, nc, R, flags, dtype, nullptr, pred_scores, pred_distri, true, stream_);
}

int evrep_dethead_train_backward_typed(const evrep_dethead_grad_level_typed *levels_host, int32_t L, int32_t B, int32_t nc,
                                       int32_t R, uint32_t flags, int32_t dtype, const float *pred_scores,
                                       const float *grad_scores, const float *grad_distri, void *stream_) {
    const uintptr_t elem = dt_size(dtype);
    if (!dethead_shape_ok(L, B, nc, R, flags) || bad_ptr(levels_host, 8) || !elem) return EVREP_EINVAL;
    if (!grad_scores && !grad_distri) return EVREP_EINVAL;             // nothing asked for
    if (misaligned(grad_scores, 4) || misaligned(grad_distri, 4)) return EVREP_EINVAL;
    if (grad_scores ? bad_ptr(pred_scores, 4) : misaligned(pred_scores, 4)) return EVREP_EINVAL;
    DetheadArgs t;
    memset(&t, 0, sizeof(t));
    int64_t total = 0, tiles = 0;
    for (int32_t l = 0; l < L; ++l) {
        const evrep_dethead_grad_level_typed &g = levels_host[l];
        if (!dethead_level(t, l, g.h, g.w, total, tiles)) return EVREP_EINVAL;
        if (grad_scores ? bad_ptr(g.gcls, elem) : g.gcls != nullptr) return EVREP_EINVAL;   // a half comes whole or not at all
        if (grad_distri ? bad_ptr(g.greg, elem) : g.greg != nullptr) return EVREP_EINVAL;
        t.gcls[l] = g.gcls; t.greg[l] = g.greg;
    }
    t.p = pred_scores; t.gs = grad_scores; t.gd = grad_distri;
    t.L = L; t.N = (int32_t)total; t.nc = nc;
    t.use_dfl = (flags & EVREP_DETHEAD_USE_DFL) ? 1 : 0;
    t.K = t.use_dfl ? R + 1 : 1;
    DETHEAD_LAUNCH(k_dethead_backward, dtype, dim3((unsigned)tiles, (unsigned)B), as_stream(stream_), t);
    LAUNCH_CHECK("k_dethead_backward");
    return EVREP_OK;
}

int evrep_dethead_train_backward(const evrep_dethead_grad_level *levels_host, int32_t L, int32_t B, int32_t nc, int32_t R,
                                 uint32_t flags, const float *pred_scores, const float *grad_scores, const float *grad_distri,
                                 void *stream_) {
    return evrep_dethead_train_backward_typed(reinterpret_cast<const evrep_dethead_grad_level_typed *>(levels_host), L, B, nc, R, flags,
                                              EVREP_DT_F32, pred_scores, grad_scores, grad_distri, stream_);
}

static inline bool step_tables_ok(const evrep_step_tensor *tensors, int32_t n_tensors, const evrep_step_chunk *chunks,
                                  int64_t n_chunks, const float *hyper) {
    if (n_tensors < 0 || n_chunks < 0 || n_chunks > INT32_MAX || bad_ptr(hyper, 4)) return false;
    if (n_tensors > 0 ? bad_ptr(tensors, 8) : misaligned(tensors, 8)) return false;
    if (n_chunks > 0 ? (bad_ptr(chunks, 8) || n_tensors < 1) : misaligned(chunks, 8)) return false;
    return true;
}

int evrep_train_step(const evrep_step_tensor *tensors, int32_t n_tensors, const evrep_step_chunk *chunks, int64_t n_chunks,
                     const float *hyper, int32_t n_groups, int32_t *amp, int32_t *applied_steps, double growth, double backoff,
                     int32_t growth_interval, uint32_t flags, void *stream_) {
    if (!step_tables_ok(tensors, n_tensors, chunks, n_chunks, hyper)) return EVREP_EINVAL;
    if (n_groups < 1 || n_groups > EVREP_STEP_MAX_GROUPS) return EVREP_EINVAL;
    if (flags & ~(uint32_t)(EVREP_STEP_ZERO_GRAD | EVREP_STEP_NO_CHECK | EVREP_STEP_KEEP_SCALE)) return EVREP_EINVAL;
    if (misaligned(amp, 4) || bad_ptr(applied_steps, 4)) return EVREP_EINVAL;
    if (amp && !(flags & EVREP_STEP_KEEP_SCALE)) {
        const auto factor = [](double v) { return v > 0.0 && v - v == 0.0; };   // finite and > 0 (NaN fails)
        if (!factor(growth) || !factor(backoff) || growth_interval < 1) return EVREP_EINVAL;
    }
    StepArgs a;
    memset(&a, 0, sizeof(a));
    a.tensors = tensors; a.chunks = chunks; a.hyper = hyper; a.amp = amp; a.applied = applied_steps;
    a.growth = growth; a.backoff = backoff; a.interval = growth_interval;
    a.n_tensors = n_tensors; a.n_groups = n_groups; a.flags = flags;
    hipStream_t stream = as_stream(stream_);
    if (n_chunks > 0 && amp && !(flags & EVREP_STEP_NO_CHECK)) {
        k_step_check<<<(unsigned)n_chunks, kThreads, 0, stream>>>(a);
        LAUNCH_CHECK("k_step_check");
    }
    if (n_chunks > 0) {
        k_step_apply<<<(unsigned)n_chunks, kThreads, 0, stream>>>(a);
        LAUNCH_CHECK("k_step_apply");
    }
    k_step_finish<<<1, kWave, 0, stream>>>(a);
    LAUNCH_CHECK("k_step_finish");
    return EVREP_OK;
}

int evrep_ema_update(const evrep_step_tensor *tensors, int32_t n_tensors, const evrep_step_chunk *chunks, int64_t n_chunks,
                     const float *hyper, void *stream_) {
    if (!step_tables_ok(tensors, n_tensors, chunks, n_chunks, hyper)) return EVREP_EINVAL;
    if (n_chunks == 0) return EVREP_OK;
    StepArgs a;
    memset(&a, 0, sizeof(a));
    a.tensors = tensors; a.chunks = chunks; a.hyper = hyper;
    a.n_tensors = n_tensors; a.ema_only = 1;
    k_step_apply<<<(unsigned)n_chunks, kThreads, 0, as_stream(stream_)>>>(a);
    LAUNCH_CHECK("k_step_apply");
    return EVREP_OK;
}

}  // extern "C"
