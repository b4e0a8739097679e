// evrep_dfl.h -- the one statement of a box side's distance under DFL (rule 1 of detector_loss.py, rule E1 of
// detector_head.py): evrep_detloss.hip and evrep_dethead.hip both include it, so the two decodes cannot drift apart.
//
// Every statement is ONE float64 operation; the float32 logits are widened exactly; exp is the double library function;
// max(a, b) is a > b ? a : b.  The including file is compiled with -ffp-contract=off and repeats it as a pragma.
#pragma once
#include "evrep_common.h"

#pragma clang fp contract(off)

namespace evrep {

__device__ inline double dl_max(double a, double b) { return a > b ? a : b; }
__device__ inline double dl_min(double a, double b) { return a < b ? a : b; }

// one side: the K logits z[0], z[step], ... z[(K - 1) * step] -> the maximum m, the sum of exponentials Z and the
// expectation d = the products (e_k / Z) * k added left to right
__device__ inline void dfl_side(const float *__restrict__ z, int step, int K, double &m, double &Z, double &d) {
    m = (double)z[0];
    for (int k = 1; k < K; ++k) m = dl_max(m, (double)z[k * step]);
    Z = 0.0;
    for (int k = 0; k < K; ++k) Z = __dadd_rn(Z, exp(__dsub_rn((double)z[k * step], m)));
    d = 0.0;
    for (int k = 0; k < K; ++k) d = __dadd_rn(d, __dmul_rn(__ddiv_rn(exp(__dsub_rn((double)z[k * step], m)), Z), (double)k));
}

}  // namespace evrep
