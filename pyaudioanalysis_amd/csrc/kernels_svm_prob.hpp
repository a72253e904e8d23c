// libsvm's multiclass_probability for two classes, shared by the onset-probability kernels (kernels_svm.hpp:
// svm_binary_proba_kernel; kernels_onset.hpp: onset_proba_kernel).
#pragma once
#include "device_common.hpp"

namespace paa {

// libsvm's multiclass_probability for k = 2 (pairwise r01 = p, r10 = 1 - p); returns the probability of class index 1.
// Kept operation by operation (no FMA contraction) so that the early-exit iteration follows libsvm's path.
#pragma clang fp contract(off)
__device__ __forceinline__ double libsvm_two_class_prob1(double r01) {
    const double r10 = 1.0 - r01;
    double Q00 = r10 * r10, Q11 = r01 * r01, Q01 = -r10 * r01;
    double p0 = 0.5, p1 = 0.5;
    const double eps = 0.005 / 2.0;
    for (int iter = 0; iter < 100; ++iter) {
        double Qp0 = 0.0, Qp1 = 0.0, pQp = 0.0;
        Qp0 += Q00 * p0; Qp0 += Q01 * p1;
        pQp += p0 * Qp0;
        Qp1 += Q01 * p0; Qp1 += Q11 * p1;
        pQp += p1 * Qp1;
        const double e0 = fabs(Qp0 - pQp), e1 = fabs(Qp1 - pQp);
        const double max_error = e1 > e0 ? e1 : e0;
        if (max_error < eps) break;
        {   // t = 0
            const double diff = (-Qp0 + pQp) / Q00;
            p0 += diff;
            pQp = (pQp + diff * (diff * Q00 + 2 * Qp0)) / (1 + diff) / (1 + diff);
            Qp0 = (Qp0 + diff * Q00) / (1 + diff);
            p0 /= (1 + diff);
            Qp1 = (Qp1 + diff * Q01) / (1 + diff);
            p1 /= (1 + diff);
        }
        {   // t = 1
            const double diff = (-Qp1 + pQp) / Q11;
            p1 += diff;
            pQp = (pQp + diff * (diff * Q11 + 2 * Qp1)) / (1 + diff) / (1 + diff);
            Qp0 = (Qp0 + diff * Q01) / (1 + diff);
            p0 /= (1 + diff);
            Qp1 = (Qp1 + diff * Q11) / (1 + diff);
            p1 /= (1 + diff);
        }
    }
    return p1;
}
#pragma clang fp contract(fast)

}  // namespace paa
