// evrep_est_bwd.hip -- the EST quantisation layer's backward with respect to its value MLP, as a keyed reduction.
//
// The MLP is f(u) = a_k u + c_k on piece k (evrep_est_table.h), and the forward writes
//   vox[b, y, x, p*C + i] = sum_n tn_n * f(u_ni),  u_ni = float32(tn_n - shift_i).
// With G = dL/dvox the gradient with respect to the table is
//   dL/da_k = sum over (n, i) with piece(u_ni) = k of G[b_n, y_n, x_n, p_n*C + i] * tn_n * u_ni
//   dL/dc_k = the same sum of                         G[b_n, y_n, x_n, p_n*C + i] * tn_n
// and autograd carries (dL/da, dL/dc) on to the six weight tensors on the host side (est.piece_coefficients).
//
// Arithmetic, fixed: g = (double)G * (double)tn is exact (two 24-bit significands); ga = g * (double)u rounds once;
// both are added to piece k in float64.  The ORDER of the additions is fixed by the source alone, so two calls on the
// same inputs return the same bits on any device, and no floating-point atomic touches memory:
//   * the stream [offsets[0], offsets[B]) is cut into slices of kEbSlice events; workgroup w of a grid of kEbGroups
//     (one wave each) takes slices w, w + kEbGroups, ... in ascending order and keeps its 2 * nseg sums in LDS;
//   * a batch of 64 events and one bin is folded per distinct piece: ballot the lanes of the first live lane's piece,
//     sum their terms (zeros elsewhere) with a fixed xor butterfly, one lane adds the two sums to the LDS table.
//     Ascending timestamps give one or two pieces per batch and bin; unsorted ones up to 64, slower and as correct;
//   * the workgroup writes the range of pieces it touched to its row of the scratch;
//   * k_est_bwd_sum adds the rows in workgroup order, one thread per output.
// Events outside the frame or with p not in {0, 1} contribute nothing.  The events are read in array order: no plan,
// no binning pass, no workspace.
#include "evrep_capi_shared.h"
#include "evrep_est_table.h"

namespace evrep {

constexpr int kEbSlice = 1024;     // events per slice (16 batches of one wave)
constexpr int kEbGroups = 512;     // workgroups of the first launch = rows of the scratch
constexpr int kEbSumThreads = 256;

static_assert(kEbSlice % kWave == 0, "a slice is a whole number of batches");

// scratch: int32 [kEbGroups][2] touched piece range {first, last} (first > last: none), then double [rows][2 * nseg]
__host__ __device__ inline size_t eb_off_rows() { return ((size_t)kEbGroups * 2 * sizeof(int32_t) + 255) & ~(size_t)255; }

__device__ inline int64_t eb_rows_used(int64_t n) {
    const int64_t slices = (n + kEbSlice - 1) / kEbSlice;
    return slices < kEbGroups ? slices : kEbGroups;
}

__device__ inline double eb_wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v = v + __shfl_xor(v, m, kWave);
    return v;                       // the same bits in every lane: each level adds the same two partial sums in both
}

struct EstBwdArgs {
    const int4 *ev;                 // rows {x, y, t, p}
    const int64_t *off;             // [B + 1]
    const float *tnorm;             // indexed like ev
    const double *seg;              // [nseg][3] {u_next, a, c}
    const uint32_t *bucket;
    const float *gout;              // (B, H, W, 2C)
    int32_t B, H, W;
};

__global__ __launch_bounds__(kWave) void k_est_bwd(EstBwdArgs a, EstParams P, int32_t *__restrict__ range,
                                                   double *__restrict__ rows) {
    extern __shared__ __align__(16) unsigned char smem[];
    double *acc = reinterpret_cast<double *>(smem);               // [nseg][2] {d/da, d/dc}
    const int lane = threadIdx.x;
    const int64_t n0 = a.off[0], n1 = a.off[a.B];
    const int64_t used = eb_rows_used(n1 - n0);
    if ((int64_t)blockIdx.x >= used) return;                       // wave-uniform: k_est_bwd_sum does not read this row
    for (int j = lane; j < 2 * P.nseg; j += kWave) acc[j] = 0.0;
    __syncthreads();
    int kfirst = P.nseg, klast = -1;                               // wave-uniform
    const int C = P.C;
    for (int64_t s = n0 + (int64_t)blockIdx.x * kEbSlice; s < n1; s += (int64_t)kEbGroups * kEbSlice) {
        const int64_t send = s + kEbSlice < n1 ? s + kEbSlice : n1;
        for (int64_t base = s; base < send; base += kWave) {
            const int64_t n = base + lane;
            bool valid = n < send;
            float tn = 0.0f;
            const float *gp = a.gout;
            if (valid) {
                const int4 e = a.ev[n];
                valid = e.x >= 0 && e.x < a.W && e.y >= 0 && e.y < a.H && (e.w == 0 || e.w == 1);
                if (valid) {
                    int lo = 0, hi = a.B;                          // the window of n: the last b with off[b] <= n (empty windows skipped)
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (a.off[mid] <= n) lo = mid; else hi = mid;
                    }
                    tn = a.tnorm[n];
                    gp += ((((size_t)lo * a.H + e.y) * (size_t)a.W + e.x) * 2 + e.w) * (size_t)C;
                }
            }
            for (int i = 0; i < C; ++i) {
                const float u = tn - P.shift[i];
                int k = -1;
                double g = 0.0, ga = 0.0;
                if (valid) {
                    k = est_piece((double)u, a.seg, a.bucket, P);
                    k = k < P.nseg ? k : P.nseg - 1;               // a well-formed bucket table never needs it: the LDS index stays inside
                    g = (double)gp[i] * (double)tn;
                    ga = g * (double)u;
                }
                unsigned long long todo = __ballot(valid);
                while (todo) {
                    const int k0 = __shfl(k, __ffsll((long long)todo) - 1, kWave);
                    const bool mine = k == k0;
                    const double sa = eb_wave_sum(mine ? ga : 0.0);
                    const double sc = eb_wave_sum(mine ? g : 0.0);
                    if (lane == 0) {
                        acc[2 * k0] = acc[2 * k0] + sa;
                        acc[2 * k0 + 1] = acc[2 * k0 + 1] + sc;
                    }
                    kfirst = k0 < kfirst ? k0 : kfirst;
                    klast = k0 > klast ? k0 : klast;
                    todo &= ~__ballot(mine);
                }
            }
        }
    }
    __syncthreads();
    if (lane == 0) { range[2 * blockIdx.x] = kfirst; range[2 * blockIdx.x + 1] = klast; }
    double *row = rows + (size_t)blockIdx.x * 2 * P.nseg;
    for (int j = 2 * kfirst + lane; j < 2 * (klast + 1); j += kWave) row[j] = acc[j];
}

// one thread per output: grad[j] = sum over the rows whose range holds piece j / 2, in row order
__global__ __launch_bounds__(kEbSumThreads) void k_est_bwd_sum(const int64_t *__restrict__ off, int B, int nseg,
                                                              const int32_t *__restrict__ range, const double *__restrict__ rows,
                                                              double *__restrict__ grad) {
    const int j = blockIdx.x * kEbSumThreads + threadIdx.x;
    if (j >= 2 * nseg) return;
    const int used = (int)eb_rows_used(off[B] - off[0]);
    const int k = j >> 1;
    double v = 0.0;
    for (int w = 0; w < used; ++w)
        if (k >= range[2 * w] && k <= range[2 * w + 1]) v = v + rows[(size_t)w * 2 * nseg + j];
    grad[j] = v;
}

}  // namespace evrep

using namespace evrep;
using evrep_host::hip_check;

extern "C" {

size_t evrep_est_backward_scratch_bytes(int64_t total_events, int32_t nseg) {
    if (total_events < 0 || nseg < 1 || nseg > EVREP_EST_BWD_MAX_SEG) return 0;
    int64_t used = (total_events + kEbSlice - 1) / kEbSlice;
    if (used > kEbGroups) used = kEbGroups;
    if (used < 1) used = 1;
    return up256(eb_off_rows() + (size_t)used * 2 * (size_t)nseg * sizeof(double));
}

int evrep_est_voxel_backward(const int32_t *events, const int64_t *offsets, int32_t B, int32_t H, int32_t W, const float *tnorm,
                             int32_t C, const double *segments, int32_t nseg, const uint32_t *buckets, int32_t nbucket, double lo,
                             double hi, const float *grad_out, double *grad_seg, void *scratch, void *stream_) {
    if (!offsets || !tnorm || !segments || !buckets || !grad_out) return EVREP_EINVAL;
    if (bad_ptr(events, 16) || bad_ptr(scratch, 16) || bad_ptr(grad_seg, 8)) return EVREP_EINVAL;
    if (B < 1 || H < 1 || W < 1 || H > EVREP_MAX_DIM || W > EVREP_MAX_DIM) return EVREP_EINVAL;
    if (C < 2 || C > kEstMaxBins || nseg < 1 || nseg > EVREP_EST_BWD_MAX_SEG || nbucket < 1 || !(hi > lo)) return EVREP_EINVAL;
    EstParams P;
    memset(&P, 0, sizeof(P));
    P.C = C; P.nseg = nseg; P.nbucket = nbucket;
    P.lo = lo; P.inv_width = (double)nbucket / (hi - lo);
    for (int i = 0; i < C; ++i) P.shift[i] = (float)((double)i / (double)(C - 1));
    EstBwdArgs a;
    a.ev = reinterpret_cast<const int4 *>(events);
    a.off = offsets;
    a.tnorm = tnorm;
    a.seg = segments;
    a.bucket = buckets;
    a.gout = grad_out;
    a.B = B; a.H = H; a.W = W;
    hipStream_t stream = as_stream(stream_);
    int32_t *range = static_cast<int32_t *>(scratch);
    double *rows = reinterpret_cast<double *>(static_cast<char *>(scratch) + eb_off_rows());
    const size_t lds = (size_t)2 * nseg * sizeof(double);
    if (lds > 64 * 1024) {  // per (function, device) opt-in, renewed per launch: a process-wide flag would miss a second device
        if (int rc = hip_check(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_est_bwd), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)lds), "hipFuncSetAttribute(k_est_bwd)")) return rc;
    }
    k_est_bwd<<<kEbGroups, kWave, lds, stream>>>(a, P, range, rows);
    LAUNCH_CHECK("k_est_bwd");
    k_est_bwd_sum<<<(2 * nseg + kEbSumThreads - 1) / kEbSumThreads, kEbSumThreads, 0, stream>>>(offsets, B, nseg, range, rows, grad_seg);
    LAUNCH_CHECK("k_est_bwd_sum");
    return EVREP_OK;
}

}  // extern "C"
