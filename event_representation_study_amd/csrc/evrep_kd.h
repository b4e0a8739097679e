// evrep_kd.h -- the one statement of a softmax at a temperature and of a row's Kullback-Leibler term, as the distillation
// losses of loss_distill.py take them (distill_loss_cls :281-292 over the classes, distill_loss_dfl :489-500 over the bins):
// evrep_detloss.hip (the box launch of evrep_detloss_distill) and evrep_detdistill.hip (its class launch) both include it.
//
// Every statement is ONE float64 operation; the float32 logits are widened exactly; x / T is a float64 division; exp and log
// are the double library functions; max(a, b) is a > b ? a : b.  The including file is compiled with -ffp-contract=off and
// repeats it as a pragma.
#pragma once
#include "evrep_common.h"
#include "evrep_dfl.h"

#pragma clang fp contract(off)

namespace evrep {

// n logits x[0] .. x[n - 1] at temperature T: m = the maximum of x_k / T, Z = the exp(x_k / T - m) added left to right
__device__ inline void kd_stats(const float *__restrict__ x, int n, double T, double &m, double &Z) {
    m = __ddiv_rn((double)x[0], T);
    for (int k = 1; k < n; ++k) m = dl_max(m, __ddiv_rn((double)x[k], T));
    Z = 0.0;
    for (int k = 0; k < n; ++k) Z = __dadd_rn(Z, exp(__dsub_rn(__ddiv_rn((double)x[k], T), m)));
}

// one probability of that softmax
__device__ inline double kd_prob(float x, double T, double m, double Z) {
    return __ddiv_rn(exp(__dsub_rn(__ddiv_rn((double)x, T), m)), Z);
}

// one term of the KL sum: pt * log(pt) - pt * log(ps), the first product 0 where pt == 0 (torch's xlogy)
__device__ inline double kd_term(double ps, double pt) {
    const double a = pt == 0.0 ? 0.0 : __dmul_rn(pt, log(pt));
    return __dsub_rn(a, __dmul_rn(pt, log(ps)));
}

// a row of student logits s and teacher logits t: kl = its terms added left to right, spt = the pt_k added left to right
__device__ inline void kd_row(const float *__restrict__ s, const float *__restrict__ t, int n, double T, double ms, double Zs,
                              double mt, double Zt, double &kl, double &spt) {
    kl = 0.0; spt = 0.0;
    for (int k = 0; k < n; ++k) {
        const double ps = kd_prob(s[k], T, ms, Zs), pt = kd_prob(t[k], T, mt, Zt);
        kl = __dadd_rn(kl, kd_term(ps, pt));
        spt = __dadd_rn(spt, pt);
    }
}

}  // namespace evrep
