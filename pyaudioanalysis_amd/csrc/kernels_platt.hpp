// The second half of libsvm's probability=True: sigmoid_train (svm.cpp), the two-parameter Newton fit of
// P(first class | dec) = 1 / (1 + exp(A dec + B)) on the held-out decision values of a class pair, FP64, one workgroup per
// PROBLEM (one class pair of one job): its l values dec[off .. off + l - 1] with a sign per value (+1: the pair's first class).
//
// platt_sigmoid_kernel follows sigmoid_train operation for operation (no contraction into fma): the targets
// (prior1 + 1) / (prior1 + 2) and 1 / (prior0 + 2), the start A = 0, B = log((prior0 + 1) / (prior1 + 1)), the two-branch forms
// of the objective and of p / q chosen by fApB >= 0, sigma = 1e-12 on the Hessian's diagonal, the stop |g1| < 1e-5 and
// |g2| < 1e-5, backtracking from step 1, halved while step >= 1e-10, with the 1e-4 sufficient-decrease test, at most 100 Newton
// iterations.  Every loop has one of those caps or runs over the l values; none runs on convergence alone.
// What differs from the serial code is the order of every sum over the values, and only that: thread t adds the values t,
// t + 256, t + 512, ... in that order, the 64 partial sums of a wave are added by an xor butterfly (every lane forms the same
// tree, addition commutes), and the four waves' sums as (w0 + w1) + (w2 + w3); sigma is added to the finished sums.  The order
// depends on l alone, so a problem's outputs are bit-identical alone or in any batch, at any grid position, run after run.
// Every thread carries the same scalars (A, B, the sums) and takes the same branches; thread 0 stores.
// dec and the signs stay in LDS: 8 l + l bytes, 72 KB at the limit of 8192 values.
#pragma once
#include "model_launch.hpp"

namespace paa {
namespace platt {

constexpr int kWaves = kThreads / 64;
static_assert(kThreads % 64 == 0 && kWaves == 4, "the sums are added as (w0 + w1) + (w2 + w3)");

// v[0 .. N-1] summed over the workgroup, every thread gets the same sums; red [N][kWaves] in LDS
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double *red, int tid) {
#pragma clang fp contract(off)
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[n] += __shfl_xor(v[n], o, 64);
    __syncthreads();                                    // the previous use of red is over
    if (tid % 64 == 0)
#pragma unroll
        for (int n = 0; n < N; ++n) red[n * kWaves + tid / 64] = v[n];
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = (red[n * kWaves] + red[n * kWaves + 1]) + (red[n * kWaves + 2] + red[n * kWaves + 3]);
}

// sigmoid_train's objective at (A, B)
__device__ __forceinline__ double objective(const double *dec, const signed char *sg, int l, double A, double B, double hi,
                                            double lo, double *red, int tid) {
#pragma clang fp contract(off)
    double s[1] = {0.0};
    for (int i = tid; i < l; i += kThreads) {
        const double t = sg[i] > 0 ? hi : lo, f = dec[i] * A + B;
        if (f >= 0.0) s[0] += t * f + log(1.0 + exp(-f));
        else s[0] += (t - 1.0) * f + log(1.0 + exp(f));
    }
    block_sum(s, red, tid);
    return s[0];
}

__global__ __launch_bounds__(kThreads) void platt_sigmoid_kernel(PlattDev p) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];                     // dec [l] | sign [l] (bytes)
    __shared__ double red[5 * kWaves];
    const int tid = threadIdx.x, prob = blockIdx.x;
    const long long off = p.off[prob];
    const int l = (int)(p.off[prob + 1] - off);
    double *dec = lds;
    signed char *sg = (signed char *)(lds + l);
    double prior[2] = {0.0, 0.0};                       // counts: exact in any order
    for (int i = tid; i < l; i += kThreads) {
        dec[i] = p.dec[off + i];
        const signed char s = p.sign[off + i];
        sg[i] = s;
        if (s > 0) prior[1] += 1.0;
        else prior[0] += 1.0;
    }
    block_sum(prior, red, tid);                         // (its barriers also publish dec and sg)
    const double prior0 = prior[0], prior1 = prior[1];
    const double hi = (prior1 + 1.0) / (prior1 + 2.0), lo = 1.0 / (prior0 + 2.0);
    double A = 0.0, B = log((prior0 + 1.0) / (prior1 + 1.0));
    double fval = objective(dec, sg, l, A, B, hi, lo, red, tid);
    int iter = 0, stop = kMaxIterations;
    for (; iter < kMaxIter; ++iter) {
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};        // h11, h22, h21, g1, g2
        for (int i = tid; i < l; i += kThreads) {
            const double d = dec[i], t = sg[i] > 0 ? hi : lo, f = d * A + B;
            double pp, q;
            if (f >= 0.0) {
                pp = exp(-f) / (1.0 + exp(-f));
                q = 1.0 / (1.0 + exp(-f));
            } else {
                pp = 1.0 / (1.0 + exp(f));
                q = exp(f) / (1.0 + exp(f));
            }
            const double d2 = pp * q, d1 = t - pp;
            s[0] += d * d * d2;
            s[1] += d2;
            s[2] += d * d2;
            s[3] += d * d1;
            s[4] += d1;
        }
        block_sum(s, red, tid);
        const double h11 = kSigma + s[0], h22 = kSigma + s[1], h21 = s[2], g1 = s[3], g2 = s[4];
        if (fabs(g1) < kEps && fabs(g2) < kEps) { stop = kConverged; break; }
        const double det = h11 * h22 - h21 * h21;
        const double dA = -(h22 * g1 - h21 * g2) / det, dB = -(-h21 * g1 + h11 * g2) / det;
        const double gd = g1 * dA + g2 * dB;
        double step = 1.0;
        for (int k = 0; k < kMaxHalvings && step >= kMinStep; ++k) {
            const double newA = A + step * dA, newB = B + step * dB;
            const double newf = objective(dec, sg, l, newA, newB, hi, lo, red, tid);
            if (newf < fval + 0.0001 * step * gd) {
                A = newA;
                B = newB;
                fval = newf;
                break;
            }
            step = step / 2.0;
        }
        if (step < kMinStep) { stop = kLineSearchFailed; break; }
    }
    if (tid == 0) {
        p.A[prob] = A;
        p.B[prob] = B;
        p.iter[prob] = iter;
        p.stop[prob] = stop;
    }
}

}  // namespace platt
}  // namespace paa
