// evrep_capi_gwd.hip -- the extern "C" surface, part 4: the GWD score, the OTMI clouds, the entropic-GW extension.
#include "evrep_capi_shared.h"

#include "evrep_gwd.hip"
#include "evrep_otmi.hip"
#include "evrep_gw.hip"

using namespace evrep;
using evrep_host::hip_check;

// The compile-time form of a pair's tile kernel.  SPLIT (clouds of <= kGwdSplitMaxD dimensions): S, T = gwd_split_steps of
// ds, dt and the LDS holds the column tile's operands; else S, T = gwd_steps and it holds the row + column tile of both clouds.
template <bool SPLIT, int S, int T>
struct GwdForm { static constexpr size_t lds = SPLIT ? (size_t)2 * (S + T) * kTile * 16 : (size_t)2 * (2 * S + 2 * T) * kTile * sizeof(float); };

// launch(GwdForm<...>()) for the form of (ds, dt): the one place that knows the forms, for the single and the batched solve.
// (Split forms first, then float32 row by row: the order of first instantiation fixes the layout of the code object.)
template <typename Launch>
static int gwd_dispatch(int ds, int dt, Launch &&launch) {
    if (gwd_use_split(ds, dt)) {
        const int ms = gwd_split_steps(ds), mt = gwd_split_steps(dt);
        if (ms == 2 && mt == 2) return launch(GwdForm<true, 2, 2>());
        if (ms == 2) return launch(GwdForm<true, 2, 6>());
        if (mt == 2) return launch(GwdForm<true, 6, 2>());
        return launch(GwdForm<true, 6, 6>());
    }
    const int ss = gwd_steps(ds), st = gwd_steps(dt);
    if (ss == 3) return st == 3 ? launch(GwdForm<false, 3, 3>()) : st == 8 ? launch(GwdForm<false, 3, 8>()) : launch(GwdForm<false, 3, 17>());
    if (ss == 8) return st == 3 ? launch(GwdForm<false, 8, 3>()) : st == 8 ? launch(GwdForm<false, 8, 8>()) : launch(GwdForm<false, 8, 17>());
    return st == 3 ? launch(GwdForm<false, 17, 3>()) : st == 8 ? launch(GwdForm<false, 17, 8>()) : launch(GwdForm<false, 17, 17>());
}

// The widest float32 instantiations need > 64 KB of dynamic LDS (the split forms never do).  The opt-in is a property of
// (function, DEVICE); it is renewed on every launch that needs it instead of being remembered in a process-wide flag (a
// second device or a second host thread would find the flag set and the attribute missing)
static int gwd_lds_opt_in(const void *kernel, size_t lds, const char *what) {
    if (lds <= 64 * 1024) return EVREP_OK;
    return hip_check(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), what);
}

// one workgroup per tile
template <bool SPLIT, int S, int T>
static int gwd_launch_tiles(GwdForm<SPLIT, S, T> form, const GwdTileArgs &P, hipStream_t stream) {
    if constexpr (SPLIT) {
        k_gwd_tiles_split<S, T><<<P.ntiles, kThreads, form.lds, stream>>>(P);
    } else {
        if (int rc = gwd_lds_opt_in(reinterpret_cast<const void *>(&k_gwd_tiles<S, T>), form.lds, "hipFuncSetAttribute(k_gwd_tiles)")) return rc;
        k_gwd_tiles<S, T><<<P.ntiles, kThreads, form.lds, stream>>>(P);
    }
    return EVREP_OK;
}
// workgroup (t, p): tile t of pair p; tile_cap = the tile count of the caller's size bounds
template <bool SPLIT, int S, int T>
static int gwd_launch_tiles_batch(GwdForm<SPLIT, S, T> form, const GwdPair *pairs, int P, int64_t tile_cap, hipStream_t stream) {
    const dim3 grid((unsigned)tile_cap, (unsigned)P);
    if constexpr (SPLIT) {
        k_gwd_tiles_split_batch<S, T><<<grid, kThreads, form.lds, stream>>>(pairs);
    } else {
        if (int rc = gwd_lds_opt_in(reinterpret_cast<const void *>(&k_gwd_tiles_batch<S, T>), form.lds, "hipFuncSetAttribute(k_gwd_tiles_batch)")) return rc;
        k_gwd_tiles_batch<S, T><<<grid, kThreads, form.lds, stream>>>(pairs);
    }
    return EVREP_OK;
}

// ---------------------------------------------------------------------------------------------- entropic GW (F5)
template <typename T>
struct GwScratch {
    T *hC1, *hC2, *ai, *bj, *Tp, *G, *Km;
    double *u, *v, *colpart, *losspart;
    int ldn, ldm;  // leading dimensions of the n-column (hC1) and m-column (hC2^T, T, G, K) matrices
    size_t bytes;
};
template <typename T>
static GwScratch<T> gw_carve(void *scratch, int64_t n, int64_t m) {
    GwScratch<T> w;
    Carver c(scratch);
    w.ldn = gw_ld((int)n, sizeof(T)); w.ldm = gw_ld((int)m, sizeof(T));
    w.hC1 = c.take<T>((size_t)n * w.ldn * sizeof(T));
    w.hC2 = c.take<T>((size_t)m * w.ldm * sizeof(T));
    w.ai = c.take<T>((size_t)n * sizeof(T));
    w.bj = c.take<T>((size_t)m * sizeof(T));
    w.Tp = c.take<T>((size_t)n * w.ldm * sizeof(T));
    w.G = c.take<T>((size_t)n * w.ldm * sizeof(T));
    w.Km = c.take<T>((size_t)n * w.ldm * sizeof(T));
    w.u = c.take<double>((size_t)n * sizeof(double));
    w.v = c.take<double>((size_t)m * sizeof(double));
    w.colpart = c.take<double>((size_t)kGwSlices * m * sizeof(double));
    w.losspart = c.take<double>((size_t)n * sizeof(double));   // one loss partial per row
    w.bytes = c.off;
    return w;
}

template <typename T>
static int gw_solve(const double *C1, int n, const double *C2, int m, const double *p, const double *q, int loss, double eps,
                    int outer_iters, int sinkhorn_iters, void *scratch, double *T_out, double *gw_out, hipStream_t stream) {
    GwScratch<T> w = gw_carve<T>(scratch, n, m);
    const dim3 ggrid((m + kGwBN - 1) / kGwBN, (n + kGwBM - 1) / kGwBM);
    const size_t nm = (size_t)n * m;
    const unsigned eblocks = (unsigned)((nm + 255) / 256);
    k_gw_init<T><<<n, kWave, 0, stream>>>(C1, n, p, loss, 1, w.hC1, w.ldn, w.ai);
    k_gw_init<T><<<m, kWave, 0, stream>>>(C2, m, q, loss, 2, w.hC2, w.ldm, w.bj);
    k_gw_outer<T><<<eblocks, 256, 0, stream>>>(p, q, n, m, w.ldm, w.Tp);
    LAUNCH_CHECK("k_gw_init");
    GwGemmArgs<T> g1;   // G = hC1 T
    memset(&g1, 0, sizeof(g1));
    g1.A = w.hC1; g1.B = w.Tp; g1.C = w.G; g1.M = n; g1.N = m; g1.K = n; g1.lda = w.ldn; g1.ldb = w.ldm; g1.ldc = w.ldm;
    GwGemmArgs<T> g2;   // exp(-2 (a_i + b_j - G hC2^T) / eps)   or the loss; w.hC2 holds h2(C2)^T, [K = m][N = m]
    memset(&g2, 0, sizeof(g2));
    g2.A = w.G; g2.B = w.hC2; g2.C = w.Km; g2.M = n; g2.N = m; g2.K = m; g2.ai = w.ai; g2.bj = w.bj;
    g2.lda = w.ldm; g2.ldb = w.ldm; g2.ldc = w.ldm;
    g2.Tplan = w.Tp; g2.inv_eps = 1.0 / eps; g2.partial = w.losspart;
    for (int it = 0; it < outer_iters; ++it) {
        k_gw_gemm<T, false, GW_EPI_STORE><<<ggrid, kThreads, 0, stream>>>(g1);
        k_gw_gemm<T, false, GW_EPI_STORE><<<ggrid, kThreads, 0, stream>>>(g2);
        k_gw_gibbs<T><<<eblocks, 256, 0, stream>>>(w.Km, w.ai, w.bj, n, m, w.ldm, 1.0 / eps);
        LAUNCH_CHECK("k_gw_gemm");
        k_gw_fill<<<(n + 255) / 256, 256, 0, stream>>>(w.u, n, 1.0 / n);
        k_gw_fill<<<(m + 255) / 256, 256, 0, stream>>>(w.v, m, 1.0 / m);
        for (int s = 0; s < sinkhorn_iters; ++s) {
            k_gw_colsum<T><<<dim3((m + kThreads - 1) / kThreads, kGwSlices), kThreads, 0, stream>>>(w.Km, w.u, n, m, w.ldm, w.colpart);
            k_gw_col_finish<<<(m + 255) / 256, 256, 0, stream>>>(w.colpart, q, m, w.v);
            k_gw_rowdot<T><<<n, kWave, 0, stream>>>(w.Km, w.v, p, m, w.ldm, w.u);
        }
        k_gw_plan<T><<<eblocks, 256, 0, stream>>>(w.Km, w.u, w.v, n, m, w.ldm, w.Tp);
        LAUNCH_CHECK("sinkhorn");
    }
    k_gw_gemm<T, false, GW_EPI_STORE><<<ggrid, kThreads, 0, stream>>>(g1);
    k_gw_gemm<T, false, GW_EPI_STORE><<<ggrid, kThreads, 0, stream>>>(g2);
    k_gw_lossrows<T><<<n, kWave, 0, stream>>>(w.Km, w.Tp, w.ai, w.bj, m, w.ldm, w.losspart);
    k_gw_loss_finish<<<1, kThreads, 0, stream>>>(w.losspart, n, gw_out);
    if (T_out) k_gw_export<T><<<eblocks, 256, 0, stream>>>(w.Tp, n, m, w.ldm, T_out);
    LAUNCH_CHECK("k_gw_loss");
    return EVREP_OK;
}

extern "C" {

// ---------------------------------------------------------------------------------------------- GWD
static int64_t pad_tile(int64_t n) { return (n + kTile - 1) / kTile * kTile; }
// bytes per point and form of a scaled cloud, whatever its dimension and form: 6 split steps x 32 B > 2 x 17 float32 steps x 4 B
constexpr size_t kGwdFormBytesMax = 192;
static_assert(kGwdFormBytesMax >= 6 * 32 && kGwdFormBytesMax >= 2 * 17 * sizeof(float), "kGwdFormBytesMax");

// scratch of one solve.  The scaled clouds are sized for the widest form, so the size depends on n and m alone.
struct GwdScratch {
    double *stat;                   // [2][kStatBlocks][2 * kGwdMaxD] partial sums, then [2][kGwdFin] final statistics
    float *YsA, *YsB, *YtA, *YtB;   // scaled clouds s and t: row + column form
    double *partial;                // per-tile, per-wave sums
    size_t bytes;
};
constexpr size_t kGwdStatPartials = (size_t)2 * kStatBlocks * 2 * kGwdMaxD;
static int64_t gwd_tiles_per_edge(int64_t n, int64_t m) { return pad_tile(n > m ? n : m) / kTile; }
static GwdScratch gwd_carve(void *scratch, int64_t n, int64_t m) {
    GwdScratch w;
    Carver c(scratch);
    const int64_t T = gwd_tiles_per_edge(n, m);
    const size_t sbytes = kGwdFormBytesMax * (size_t)pad_tile(n), tbytes = kGwdFormBytesMax * (size_t)pad_tile(m);
    w.stat = c.take<double>((kGwdStatPartials + 2 * kGwdFin) * sizeof(double));
    w.YsA = c.take<float>(sbytes);
    w.YsB = c.take<float>(sbytes);
    w.YtA = c.take<float>(tbytes);
    w.YtB = c.take<float>(tbytes);
    w.partial = c.take<double>((size_t)(T * (T + 1) / 2) * kWaves * sizeof(double));
    w.bytes = c.off;
    return w;
}

size_t evrep_gwd_scratch_bytes(int64_t n, int64_t m) {
    if (n <= 0 || m <= 0) return 0;
    return gwd_carve(nullptr, n, m).bytes;
}

int evrep_gwd_padded_l1(const double *Xs, int64_t n, int32_t ds, const double *Xt, int64_t m, int32_t dt, double h,
                        void *scratch, double *cost, void *stream_) {
    if (!Xs || !Xt || !cost || n <= 0 || m <= 0 || ds <= 0 || dt <= 0 || ds > kGwdMaxD || dt > kGwdMaxD)
        return EVREP_EINVAL;
    if (!(h > 0.0) || bad_ptr(scratch, 256)) return EVREP_EINVAL;
    hipStream_t stream = as_stream(stream_);
    const int64_t L = n > m ? n : m;
    const int T = (int)gwd_tiles_per_edge(n, m);
    if ((int64_t)T * (T + 1) / 2 * kWaves > 0x7fffffff) return EVREP_EINVAL;
    const GwdScratch w = gwd_carve(scratch, n, m);
    double *fin = w.stat + kGwdStatPartials;
    const int64_t npad = pad_tile(n), mpad = pad_tile(m);
    // five launches per solve: the clouds' partial sums; their final statistics; one scaling launch for both clouds; the
    // tiles; the final sum
    k_gwd_stats<<<dim3(kStatBlocks, 2), kThreads, 0, stream>>>(Xs, n, ds, Xt, m, dt, w.stat);
    LAUNCH_CHECK("k_gwd_stats");
    const int sblocks = (int)((npad + kThreads - 1) / kThreads), tblocks = (int)((mpad + kThreads - 1) / kThreads);
    k_gwd_stats_finish<<<2, 64, 0, stream>>>(Xs, Xt, w.stat, n, ds, m, dt, h, fin);
    LAUNCH_CHECK("k_gwd_stats_finish");
    // the split form spreads a point's chunks over blockIdx.z
    const int prep_z = gwd_use_split(ds, dt) ? 2 * gwd_split_steps(ds > dt ? ds : dt) : 1;
    k_gwd_prep<<<dim3(sblocks + tblocks, 1, prep_z), kThreads, 0, stream>>>(Xs, n, ds, npad, Xt, m, dt, mpad, fin, sblocks, w.YsA, w.YsB, w.YtA, w.YtB);
    LAUNCH_CHECK("k_gwd_prep");
    GwdTileArgs P;
    P.YsA = w.YsA; P.YsB = w.YsB; P.YtA = w.YtA; P.YtB = w.YtB; P.n = n; P.m = m; P.npad = npad; P.mpad = mpad;
    P.T = T; P.ntiles = T * (T + 1) / 2; P.partial = w.partial;
    if (int rc = gwd_dispatch(ds, dt, [&](auto form) { return gwd_launch_tiles(form, P, stream); })) return rc;
    LAUNCH_CHECK("k_gwd_tiles");
    k_gwd_finish<<<1, 1024, 0, stream>>>(w.partial, P.ntiles * kWaves, (double)L, cost);
    LAUNCH_CHECK("k_gwd_finish");
    return EVREP_OK;
}

size_t evrep_gwd_batch_scratch_bytes(int32_t P, int32_t ds, int32_t dt, int64_t n_cap, int64_t m_cap) {
    if (P <= 0 || n_cap <= 0 || m_cap <= 0 || ds <= 0 || dt <= 0 || ds > kGwdMaxD || dt > kGwdMaxD) return 0;
    return gwd_batch_layout(P, ds, dt, n_cap, m_cap).bytes;
}

int evrep_gwd_padded_l1_batch(int32_t P, const double *Xs, const int64_t *xs_row, const int64_t *n, int32_t ds,
                              const double *Xt, const int64_t *xt_row, const int64_t *m, int32_t dt, int64_t n_cap,
                              int64_t m_cap, double h, void *scratch, double *costs, void *stream_) {
    if (P <= 0 || P > 65535 || !Xs || !Xt || !n || !m || !costs) return EVREP_EINVAL;
    if (ds <= 0 || dt <= 0 || ds > kGwdMaxD || dt > kGwdMaxD || n_cap <= 0 || m_cap <= 0 || !(h > 0.0)) return EVREP_EINVAL;
    if (bad_ptr(scratch, 256)) return EVREP_EINVAL;
    const int64_t Tc = gwd_tiles_per_edge(n_cap, m_cap);
    if (Tc * (Tc + 1) / 2 * kWaves > 0x7fffffff) return EVREP_EINVAL;
    hipStream_t stream = as_stream(stream_);
    const GwdBatchLayout L = gwd_batch_layout(P, ds, dt, n_cap, m_cap);
    GwdBatchArgs B;
    B.Xs = Xs; B.Xt = Xt; B.xs_row = xs_row; B.xt_row = xt_row; B.n = n; B.m = m; B.P = P; B.ds = ds; B.dt = dt;
    B.n_cap = n_cap; B.m_cap = m_cap;
    B.scratch = static_cast<char *>(scratch);
    B.pairs = reinterpret_cast<GwdPair *>(B.scratch + L.off_pairs);
    B.total_tiles = reinterpret_cast<int64_t *>(B.scratch + L.off_total);
    B.partial = reinterpret_cast<double *>(B.scratch + L.off_partial);
    // six launches for ALL pairs: the pair table; the clouds' partial sums; their final statistics; the scaling pass; the
    // tiles (a grid sized by the caller's bounds, so no size has to be known on the host); the final sums
    k_gwd_batch_setup<<<1, kThreads, 0, stream>>>(B);
    LAUNCH_CHECK("k_gwd_batch_setup");
    k_gwd_stats_batch<<<dim3(kStatBlocks, 2, P), kThreads, 0, stream>>>(B.pairs, ds, dt);
    LAUNCH_CHECK("k_gwd_stats_batch");
    const int sblocks = (int)((pad_tile(n_cap) + kThreads - 1) / kThreads), tblocks = (int)((pad_tile(m_cap) + kThreads - 1) / kThreads);
    k_gwd_stats_finish_batch<<<dim3(2, P), 64, 0, stream>>>(B.pairs, ds, dt, h);
    LAUNCH_CHECK("k_gwd_stats_finish_batch");
    // a point's chunks over blockIdx.z: all of them for a few pairs (the launch is latency-bound), three slices for many
    // (183 000 tiny blocks cost more to dispatch than they work: 144 pairs 5.81 -> 5.64 ms)
    int prep_z = gwd_use_split(ds, dt) ? 2 * gwd_split_steps(ds > dt ? ds : dt) : 1;
    if (P >= 8 && prep_z > 3) prep_z = 3;
    k_gwd_prep_batch<<<dim3(sblocks + tblocks, P, prep_z), kThreads, 0, stream>>>(B.pairs, ds, dt, sblocks);
    LAUNCH_CHECK("k_gwd_prep_batch");
    const int64_t tile_cap = Tc * (Tc + 1) / 2;
    if (int rc = gwd_dispatch(ds, dt, [&](auto form) { return gwd_launch_tiles_batch(form, B.pairs, P, tile_cap, stream); })) return rc;
    LAUNCH_CHECK("k_gwd_tiles_batch");
    k_gwd_finish_batch<<<P, 1024, 0, stream>>>(B.pairs, costs);
    LAUNCH_CHECK("k_gwd_finish_batch");
    return EVREP_OK;
}

size_t evrep_otmi_scratch_bytes(int32_t count) {
    if (count <= 0) return 0;
    const size_t a = otmi_ev_scratch_bytes(count), b = otmi_rep_scratch_bytes(count);
    return up256(a > b ? a : b);
}

int evrep_otmi_event_clouds(const int32_t *events, const int64_t *offsets, int32_t B, int32_t height, int32_t width,
                            int64_t cap, double *Xs, int64_t *n_out, int32_t *quad_out, void *scratch, void *stream_) {
    if (!offsets || !Xs || !n_out || !quad_out || B <= 0 || B > 65535 || height <= 1 || width <= 1 || cap <= 0) return EVREP_EINVAL;
    if (bad_ptr(events, 16) || bad_ptr(scratch, 16)) return EVREP_EINVAL;
    hipStream_t stream = as_stream(stream_);
    const int4 *ev = reinterpret_cast<const int4 *>(events);
    const OtmiEvScratch w = otmi_ev_scratch(scratch, B);
    const dim3 grid(kOtmiEvSlices, B);
    k_otmi_ev_stats<<<grid, kOtmiThreads, 0, stream>>>(ev, offsets, height, width, w);
    LAUNCH_CHECK("k_otmi_ev_stats");
    k_otmi_ev_plan<<<B, 64, 0, stream>>>(w, quad_out);
    LAUNCH_CHECK("k_otmi_ev_plan");
    k_otmi_ev_rows<false><<<grid, kOtmiThreads, 0, stream>>>(ev, offsets, height, width, cap, w, Xs, n_out);
    LAUNCH_CHECK("k_otmi_ev_rows<count>");
    k_otmi_ev_rows<true><<<grid, kOtmiThreads, 0, stream>>>(ev, offsets, height, width, cap, w, Xs, n_out);
    LAUNCH_CHECK("k_otmi_ev_rows<write>");
    return EVREP_OK;
}

int evrep_otmi_rep_clouds(const void *rep, int32_t rep_dtype, int32_t items, int32_t B, int32_t S, int32_t C,
                          const int32_t *quad, int64_t m_cap, double *Xt, int64_t *m_out, void *scratch, void *stream_) {
    if (!rep || !quad || !Xt || !m_out || items <= 0 || items > 65535 || B <= 0 || S < 4 || C <= 0 || C + 2 > kGwdMaxD || m_cap <= 0)
        return EVREP_EINVAL;
    if (!is_float_dtype(rep_dtype) || bad_ptr(scratch, 16)) return EVREP_EINVAL;
    hipStream_t stream = as_stream(stream_);
    uint32_t *cnt = static_cast<uint32_t *>(scratch);
    const dim3 grid(kOtmiRepSlices, 3, items);
#define OTMI_REP(T)                                                                                                          \
    do {                                                                                                                     \
        k_otmi_rep<T, false><<<grid, kOtmiThreads, 0, stream>>>(static_cast<const T *>(rep), B, S, C, quad, m_cap, cnt, Xt, m_out); \
        k_otmi_rep<T, true><<<grid, kOtmiThreads, 0, stream>>>(static_cast<const T *>(rep), B, S, C, quad, m_cap, cnt, Xt, m_out);  \
    } while (0)
    if (rep_dtype == EVREP_F64) OTMI_REP(double); else OTMI_REP(float);
#undef OTMI_REP
    LAUNCH_CHECK("k_otmi_rep");
    return EVREP_OK;
}

int evrep_otmi_rep_clouds_bank(const void *base, const void *bank, int32_t dtype, int32_t B, int32_t S, int32_t C, int32_t R,
                               int32_t slot, const int32_t *cand, int32_t n_cand, const int32_t *quad, int64_t m_cap,
                               double *Xt, int64_t *m_out, void *scratch, void *stream_) {
    if (!base || !bank || !cand || !quad || !Xt || !m_out || B <= 0 || n_cand <= 0 || S < 4 || C <= 0 || C + 2 > kGwdMaxD ||
        R <= 0 || m_cap <= 0 || slot < 0 || slot >= C)
        return EVREP_EINVAL;
    if (!is_float_dtype(dtype) || bad_ptr(scratch, 16)) return EVREP_EINVAL;
    if ((int64_t)n_cand * B > 65535) return EVREP_EINVAL;
    for (int32_t j = 0; j < n_cand; ++j)
        if (cand[j] < 0 || cand[j] >= R) return EVREP_EINVAL;
    hipStream_t stream = as_stream(stream_);
    uint32_t *cnt = static_cast<uint32_t *>(scratch);
    const size_t lds = (size_t)kOtmiBankWaves * otmi_bank_lds_doubles(C + 2) * sizeof(double);
    // the candidates' bank channels reach the device as kernel arguments (cand is HOST memory and is not read after the
    // call returns), kOtmiBankMaxCand per pair of launches
    OtmiBankCands cs;
    for (int32_t first = 0; first < n_cand; first += kOtmiBankMaxCand) {
        cs.first = first;
        cs.n = n_cand - first < kOtmiBankMaxCand ? n_cand - first : kOtmiBankMaxCand;
        for (int32_t j = 0; j < kOtmiBankMaxCand; ++j) cs.idx[j] = j < cs.n ? cand[first + j] : 0;
        const int groups = (cs.n + kOtmiBankGroup - 1) / kOtmiBankGroup;
        const dim3 grid(kOtmiRepSlices / kOtmiBankWaves, 3, (unsigned)(groups * B));
#define OTMI_BANK(T)                                                                                                          \
    do {                                                                                                                      \
        k_otmi_rep_bank<T, false><<<grid, kOtmiBankWaves * 64, 0, stream>>>(static_cast<const T *>(base), static_cast<const T *>(bank), \
                                                                            B, S, C, R, slot, cs, quad, m_cap, cnt, Xt, m_out);          \
        k_otmi_rep_bank<T, true><<<grid, kOtmiBankWaves * 64, lds, stream>>>(static_cast<const T *>(base), static_cast<const T *>(bank), \
                                                                             B, S, C, R, slot, cs, quad, m_cap, cnt, Xt, m_out);         \
    } while (0)
        if (dtype == EVREP_F64) OTMI_BANK(double); else OTMI_BANK(float);
#undef OTMI_BANK
        LAUNCH_CHECK("k_otmi_rep_bank");
    }
    return EVREP_OK;
}

size_t evrep_gw_scratch_bytes(int64_t n, int64_t m, int32_t precision) {
    if (n <= 0 || m <= 0) return 0;
    return precision == EVREP_F32 ? gw_carve<float>(nullptr, n, m).bytes : gw_carve<double>(nullptr, n, m).bytes;
}

int evrep_entropic_gw(const double *C1, int64_t n, const double *C2, int64_t m, const double *p, const double *q,
                      int32_t loss, double epsilon, int32_t outer_iters, int32_t sinkhorn_iters, int32_t precision,
                      void *scratch, double *T_out, double *gw_out, void *stream_) {
    if (!C1 || !C2 || !p || !q || !gw_out || n <= 0 || m <= 0 || n > 46340 || m > 46340) return EVREP_EINVAL;
    if ((loss != 0 && loss != 1) || !(epsilon > 0.0) || outer_iters < 0 || sinkhorn_iters < 1) return EVREP_EINVAL;
    if (!is_float_dtype(precision) || bad_ptr(scratch, 256)) return EVREP_EINVAL;
    hipStream_t stream = as_stream(stream_);
    if (precision == EVREP_F32)
        return gw_solve<float>(C1, (int)n, C2, (int)m, p, q, loss, epsilon, outer_iters, sinkhorn_iters, scratch, T_out, gw_out, stream);
    return gw_solve<double>(C1, (int)n, C2, (int)m, p, q, loss, epsilon, outer_iters, sinkhorn_iters, scratch, T_out, gw_out, stream);
}

}  // extern "C"
