// evrep_est_table.h -- the EST value MLP as its exact piecewise-linear table, shared by the forward builder (k_est,
// evrep_builders.hip) and the backward reduction (evrep_est_bwd.hip): both must select the SAME piece for the same u.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "evrep.h"

namespace evrep {

constexpr int kEstMaxBins = EVREP_MAX_CHANNELS / 2;

struct EstParams {
    int32_t C, nseg, nbucket, pad;
    double lo, inv_width;          // bucket = (u - lo) * inv_width
    float shift[kEstMaxBins];      // float32(i / (C - 1)), as `t - i_bin / (C - 1)` rounds it (:167)
};

// the piece of u: segment k covers u < seg[3k] (ascending).  A bucketed hint, then a forward walk.
__device__ inline int est_piece(double ud, const double *__restrict__ seg, const uint32_t *__restrict__ bucket,
                                const EstParams &P) {
    int g = (int)((ud - P.lo) * P.inv_width);
    g = g < 0 ? 0 : (g >= P.nbucket ? P.nbucket - 1 : g);
    int k = (int)bucket[g];
    while (k + 1 < P.nseg && ud >= seg[3 * k]) ++k;
    return k;
}

}  // namespace evrep
