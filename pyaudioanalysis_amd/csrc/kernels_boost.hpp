// The loss side of fitting audioTrainTest.train_gradient_boosting (audioTrainTest.py:181-199; the sweep of evaluate_classifier
// :631-700) on the device: scikit-learn 1.7.2's GradientBoostingClassifier with the log-loss, per stage and job the negative
// gradients that the stage's trees (kernels_treefit.hpp, CRIT = kFriedman) are fitted to, and the mean loss of the stage before,
// which is train_score_[stage - 1] (sklearn/_loss/_loss.pyx.tp: CyHalfMultinomialLoss / CyHalfBinomialLoss; ensemble/_gb.py
// _fit_stage, _fit_stages):
//  * K > 2: max = the row's largest raw value (the first one wins), sum = 0 + exp(raw_0 - max) + exp(raw_1 - max) + ... in class
//    order, p_k = exp(raw_k - max) / sum, residual_k = -(p_k - (y == k)); loss = log(sum) + max - raw_y;
//  * K = 2: one output; e = exp(-raw), residual = -(((1 - y) - y e) / (1 + e)) for raw > -37, else -(exp(raw) - y); loss =
//    log1pexp(raw) - y raw with scikit-learn's five ranges, and train_score_ carries the factor 2 of _fit_stages;
//  * train_score_ = (sum of the rows' losses) / n.
// Raw predictions and residuals are [k_out][n] per job (class-major: a tree reads and steps one contiguous list).  One workgroup per
// job.  THE ORDER OF THE LOSS SUM IS FIXED: the job's rows are cut into 256 consecutive chunks of ceil(n / 256) rows, thread t adds
// chunk t serially from 0.0 in row order, the 256 partial sums are added by a xor butterfly within each wave (offsets 32 .. 1) and
// the four wave sums as ((s0 + s1) + s2) + s3 -- the tree builder's shape; there is no float atomic.  The exponentials are taken
// twice (for the sum, then per class) so that no row needs a private array: no scratch at 64 classes.
#pragma once
#include "device_common.hpp"
#include "model_launch.hpp"

namespace paa {
namespace boost {

#pragma clang fp contract(off)

// _loss.pyx.tp: log1pexp
__device__ __forceinline__ double log1pexp(double x) {
    if (x <= -37.0) return exp(x);
    if (x <= -2.0) return log1p(exp(x));
    if (x <= 18.0) return log(1.0 + exp(x));
    if (x <= 33.3) return x + exp(-x);
    return x;
}

__global__ __launch_bounds__(kThreads) void boost_gradient_kernel(BoostDev m, int stage) {
    __shared__ double s_d[kThreads / kWave];
    const BoostJob job = m.jobs[blockIdx.x];
    if (stage > job.n_stages) return;                               // (uniform: the job's last loss is written at stage == n_stages)
    const int tid = threadIdx.x, n = job.n, K = job.k, k_out = K == 2 ? 1 : K;
    const int *lab = m.label + job.off;
    double *raw = m.raw + job.r_off, *res = m.resid + job.r_off;
    const bool fit = stage < job.n_stages;
    const int chunk = (n + kThreads - 1) / kThreads, c0 = min(n, tid * chunk), c1 = min(n, c0 + chunk);
    double loss = 0.0;
    for (int i = c0; i < c1; ++i) {
        const int y = lab[i];
        if (stage == 0)
            for (int k = 0; k < k_out; ++k) raw[(long long)k * n + i] = m.init[job.init_off + k];
        if (k_out == 1) {
            const double z = raw[i], yd = (double)y;
            loss = loss + (log1pexp(z) - yd * z);
            if (fit) {
                double g;
                if (z > -37.0) {
                    const double e = exp(-z);
                    g = ((1.0 - yd) - yd * e) / (1.0 + e);
                } else {
                    g = exp(z) - yd;
                }
                res[i] = -g;
            }
        } else {
            double top = raw[i];
            for (int k = 1; k < K; ++k) {
                const double v = raw[(long long)k * n + i];
                if (top < v) top = v;
            }
            double sum = 0.0;
            for (int k = 0; k < K; ++k) sum = sum + exp(raw[(long long)k * n + i] - top);
            loss = loss + ((log(sum) + top) - raw[(long long)y * n + i]);
            if (fit)
                for (int k = 0; k < K; ++k) {
                    const double p = exp(raw[(long long)k * n + i] - top) / sum;
                    res[(long long)k * n + i] = -(p - (y == k ? 1.0 : 0.0));
                }
        }
    }
    if (stage == 0) return;                                         // (uniform) no stage before
    const int lane = tid % kWave, wave = tid / kWave;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) loss = loss + __shfl_xor(loss, o, kWave);
    if (lane == 0) s_d[wave] = loss;
    __syncthreads();
    if (tid == 0) {
        const double total = ((s_d[0] + s_d[1]) + s_d[2]) + s_d[3];
        const double mean = total / (double)n;
        m.loss[job.loss_off + stage - 1] = k_out == 1 ? 2.0 * mean : mean;
    }
}

#pragma clang fp contract(fast)

}  // namespace boost
}  // namespace paa
