// Multi-class probabilistic SVC over many feature vectors: what audioTrainTest.classifier_wrapper (audioTrainTest.py:84-93)
// asks scikit-learn for once per mid-term window (audioSegmentation.mid_term_file_classification, :586-591) or once per file
// (audioTrainTest.file_classification, :1091-1095) -- predict() and predict_proba() of the shipped RBF SVC models.
// The arithmetic is libsvm's (sklearn/svm/src/libsvm/svm.cpp, a third-party dependency of the reference, scikit-learn >= 0.24
// per requirements.txt; its published algorithm is restated here and the GPU tests compare with the installed scikit-learn):
//  * svm_predict_values: kernel value of every support vector (dense k_function: RBF exp(-gamma sum_d (s_d - x_d)^2) in the
//    difference form, linear sum_d s_d x_d), then for every pair i < j of classes
//    dec_ij = sum_{s in i} sv_coef[j-1][s] K_s + sum_{s in j} sv_coef[i][s] K_s - rho[p];
//  * svm_predict: a positive dec_ij votes for i, otherwise for j; the first class with the most votes wins;
//  * svm_predict_probability: r_ij = sigmoid_predict(dec_ij, probA[p], probB[p]) clipped to [1e-7, 1 - 1e-7], r_ji = 1 - r_ij,
//    then multiclass_probability (max_iter = max(100, k), eps = 0.005 / k) -- kept operation by operation so that the
//    iteration count and early exit follow libsvm's.
// Two kernels: svc_class_sums_kernel does the O(windows x support vectors x dims) part and writes, per window, the per-class
// partial sums A[c][r] = sum_{s in c} sv_coef[r][s] K_s; svc_proba_kernel (one thread per window) forms dec_ij = A[i][j-1] +
// A[j][i] - rho, the votes and the probabilities.
#pragma once
#include "kernels_kv.hpp"
#include "model_launch.hpp"

namespace paa {
namespace svc {

// ---- kernel values and per-class sums ---------------------------------------------------------------------------------
// The lane split of kernels_kv.hpp with kWinPerGroup windows per group and the support vectors as rows; the tile's dual
// coefficients are staged beside it.  Lane l accumulates rows l and l + 8 of sv_coef for the current class; at the end of a
// class's range the rows are written to A.
using kv::group_sum;
using kv::kGroupLanes;
using kv::kMaxM;
using kv::kThreads;
using kv::kTile;
constexpr int kWinPerGroup = 2;
constexpr int kWinPerBlock = kThreads / kGroupLanes * kWinPerGroup;   // 32
static_assert(kMaxDims <= kv::kMaxDims && kMaxClasses - 1 <= 2 * kGroupLanes, "the model limits fit the lane split");

__global__ __launch_bounds__(kThreads) void svc_class_sums_kernel(SvcDev m, const double *__restrict__ feats, long long ld,
                                                                  long long n_vec, const double *__restrict__ mean,
                                                                  const double *__restrict__ scale, double *__restrict__ sums) {
    __shared__ double tile[kTile * kMaxDims];
    __shared__ double coef[(kMaxClasses - 1) * kTile];
    const int tid = threadIdx.x, lane = tid % kGroupLanes, group = tid / kGroupLanes;
    const int M = (m.n_dims + kGroupLanes - 1) / kGroupLanes, pitch = M * kGroupLanes;
    const int k = m.k, rows = k - 1;
    const long long w0 = (long long)blockIdx.x * kWinPerBlock + group * kWinPerGroup;
    double x[kWinPerGroup][kMaxM];
#pragma unroll
    for (int w = 0; w < kWinPerGroup; ++w) {
#pragma unroll
        for (int i = 0; i < kMaxM; ++i) {
            const int d = lane + kGroupLanes * i;
            x[w][i] = (i < M && d < m.n_dims && w0 + w < n_vec) ? (feats[(long long)d * ld + w0 + w] - mean[d]) / scale[d] : 0.0;
        }
    }
    double acc[kWinPerGroup][2] = {{0.0, 0.0}, {0.0, 0.0}};
    const int r0 = lane, r1 = lane + kGroupLanes;
    int cls = 0;
    auto flush = [&]() {          // class cls is complete: A[w][cls][r] for this lane's rows
#pragma unroll
        for (int w = 0; w < kWinPerGroup; ++w) {
            if (w0 + w < n_vec) {
                double *a = sums + (w0 + w) * (long long)(k * rows) + cls * rows;
                if (r0 < rows) a[r0] = acc[w][0];
                if (r1 < rows) a[r1] = acc[w][1];
            }
            acc[w][0] = 0.0;
            acc[w][1] = 0.0;
        }
        ++cls;
    };
    while (cls < k && m.class_end[cls] == 0) flush();          // classes without support vectors
    for (int base = 0; base < m.n_sv; base += kTile) {
        __syncthreads();
        kv::stage_rows(tile, m.sv, base, m.n_sv, m.n_dims, pitch, tid);
        for (int i = tid; i < rows * kTile; i += kThreads) {
            const int r = i / kTile, s = base + i % kTile;
            coef[i] = s < m.n_sv ? m.coef[(long long)r * m.n_sv + s] : 0.0;
        }
        __syncthreads();
        const int cnt = min(kTile, m.n_sv - base);
        for (int j = 0; j < cnt; ++j) {
            const double *t = tile + j * pitch + lane;
            double p[kWinPerGroup] = {0.0, 0.0};
            if (m.rbf) {
#pragma unroll
                for (int i = 0; i < kMaxM; ++i) {
                    if (i < M) {
                        const double s = t[kGroupLanes * i];
#pragma unroll
                        for (int w = 0; w < kWinPerGroup; ++w) { const double df = s - x[w][i]; p[w] = fma(df, df, p[w]); }
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < kMaxM; ++i) {
                    if (i < M) {
                        const double s = t[kGroupLanes * i];
#pragma unroll
                        for (int w = 0; w < kWinPerGroup; ++w) p[w] = fma(s, x[w][i], p[w]);
                    }
                }
            }
            const double c0 = r0 < rows ? coef[r0 * kTile + j] : 0.0, c1 = r1 < rows ? coef[r1 * kTile + j] : 0.0;
#pragma unroll
            for (int w = 0; w < kWinPerGroup; ++w) {
                double kv = group_sum(p[w]);
                if (m.rbf) kv = exp(-m.gamma * kv);
                acc[w][0] = fma(c0, kv, acc[w][0]);
                acc[w][1] = fma(c1, kv, acc[w][1]);
            }
            while (cls < k && m.class_end[cls] == base + j + 1) flush();   // last vector of class cls (and empty ones after it)
        }
    }
    while (cls < k) flush();
}

// ---- decision values, votes, probabilities: one thread per window ----------------------------------------------------------
// Q (k x k), p and Qp live in LDS, column `tid` of a [k * k + 2 k][threads] array (thread-private, conflict-free); the
// iteration's loops over t stay rolled, so that no k x k block of Q is hoisted into registers.
template <int K>
constexpr int proba_threads() { return (K * K + 2 * K) * 8 * 64 <= 48 * 1024 ? 64 : (K * K + 2 * K) * 8 * 32 <= 48 * 1024 ? 32 : 16; }

#pragma clang fp contract(off)
__device__ __forceinline__ double sigmoid_predict(double dec, double A, double B) {
    const double fApB = dec * A + B;
    // 1 - p_i fails when p_i ~ 1: the equivalent stable forms (svm.cpp sigmoid_predict)
    if (fApB >= 0) return exp(-fApB) / (1.0 + exp(-fApB));
    return 1.0 / (1 + exp(fApB));
}

template <int K>
__global__ __launch_bounds__(proba_threads<K>()) void svc_proba_kernel(SvcDev m, long long n_vec, const double *__restrict__ sums,
                                                                        int *__restrict__ label, double *__restrict__ proba) {
    constexpr int T = proba_threads<K>();
    constexpr int R = K - 1;
    __shared__ double Qs[(K * K + 2 * K) * T];
    const int tid = threadIdx.x;
    const long long w = (long long)blockIdx.x * T + tid;
    if (w >= n_vec) return;
    const double *a = sums + w * (K * R);
    auto Q = [&](int t, int j) -> double & { return Qs[(t * K + j) * T + tid]; };
    auto P = [&](int t) -> double & { return Qs[(K * K + t) * T + tid]; };
    auto QP = [&](int t) -> double & { return Qs[(K * K + K + t) * T + tid]; };
    // votes are counted in the Qp column (exact small integers) before the iteration needs it
#pragma unroll
    for (int i = 0; i < K; ++i) { QP(i) = 0.0; Q(i, i) = 0.0; }
    // Q[t][t] = sum_{j != t} r[j][t]^2 in ascending j: the pair loop below meets the terms of row t in exactly that order
    // (pairs (i, t), i < t, in earlier rows of the loop; then (t, j), j > t)
    int p = 0;
#pragma unroll 1
    for (int i = 0; i < K; ++i) {
#pragma unroll 1
        for (int j = i + 1; j < K; ++j) {
            const double dec = (a[i * R + (j - 1)] + a[j * R + i]) - m.rho[p];
            QP(dec > 0 ? i : j) += 1.0;
            const double min_prob = 1e-7;
            const double rij = fmin(fmax(sigmoid_predict(dec, m.prob_a[p], m.prob_b[p]), min_prob), 1 - min_prob);
            const double rji = 1 - rij;
            Q(i, i) += rji * rji;          // r[j][i]^2
            Q(j, j) += rij * rij;          // r[i][j]^2
            Q(i, j) = -rji * rij;          // Q[t][j] = -r[j][t] * r[t][j] (t < j), mirrored
            Q(j, i) = Q(i, j);
            ++p;
        }
    }
    int best = 0;
    double most = QP(0);
#pragma unroll
    for (int i = 1; i < K; ++i)
        if (QP(i) > most) { most = QP(i); best = i; }
    label[w] = best;
#pragma unroll
    for (int t = 0; t < K; ++t) P(t) = 1.0 / K;
    const int max_iter = K > 100 ? K : 100;
    const double eps = 0.005 / K;
    for (int iter = 0; iter < max_iter; ++iter) {
        double pQp = 0;
#pragma unroll 1
        for (int t = 0; t < K; ++t) {
            double qp = 0;
#pragma unroll
            for (int j = 0; j < K; ++j) qp += Q(t, j) * P(j);
            QP(t) = qp;
            pQp += P(t) * qp;
        }
        double max_error = 0;
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const double error = fabs(QP(t) - pQp);
            if (error > max_error) max_error = error;
        }
        if (max_error < eps) break;
#pragma unroll 1
        for (int t = 0; t < K; ++t) {
            const double Qtt = Q(t, t), Qpt = QP(t);
            const double diff = (-Qpt + pQp) / Qtt;
            P(t) += diff;
            pQp = (pQp + diff * (diff * Qtt + 2 * Qpt)) / (1 + diff) / (1 + diff);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                QP(j) = (QP(j) + diff * Q(t, j)) / (1 + diff);
                P(j) /= (1 + diff);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < K; ++t) proba[w * K + t] = P(t);
}
#pragma clang fp contract(fast)

}  // namespace svc
}  // namespace paa
