// A bank of epsilon-SVR models over many feature vectors: what audioTrainTest.regression_wrapper (audioTrainTest.py:96-111)
// asks scikit-learn for once per vector and model -- file_regression (:1099-1151) applies every model_name_* model (one per
// target value, each with its own MEANS file) to one long-term vector, evaluate_regression (:774-855) a hundred models per
// parameter value to the same sample matrix.  The arithmetic is libsvm's svm_predict_values for an EPSILON_SVR model
// (sklearn/svm/src/libsvm/svm.cpp, a third-party dependency of the reference; its published algorithm is restated here and
// the GPU tests compare with the installed scikit-learn):
//   out[m][v] = sum_s coef[s] K(sv_s, (x_v - mean_m) / std_m) - rho_m,   s over model m's support vectors IN THEIR ORDER,
// K the dense k_function: RBF exp(-gamma sum_d (s_d - x_d)^2) in the difference form, linear sum_d s_d x_d -- on the lane
// split of kernels_kv.hpp with kWinPerGroup windows per group and the support vectors as rows.
// Its own is the shape of the work: the grid is window tiles x chunks of kModelChunk models; a workgroup walks the
// models of its chunk one after the other, forms the standardised vectors on the load path once per model (the models of a bank keep
// their own mean / std) and keeps the registers when a model's mean / std equal its predecessor's bit for bit (same_prev,
// set by the host: the evaluate_regression case).  One coefficient per support vector, one running sum per window: every
// value is a fixed-order sum owned by one lane group -- no atomics, no reduction across workgroups -- and depends neither on
// the window's place in the batch, nor on n_vec, ld, the chunking or the other models of the bank.  A model without support
// vectors gives 0 - rho.  Non-finite inputs are not validated (as in the SVC kernel): they propagate by IEEE rules.
#pragma once
#include "kernels_kv.hpp"
#include "model_launch.hpp"

namespace paa {
namespace svr {

using kv::group_sum;
using kv::kGroupLanes;
using kv::kMaxM;
using kv::kThreads;
using kv::kTile;
constexpr int kWinPerGroup = 2;
constexpr int kWinPerBlock = kThreads / kGroupLanes * kWinPerGroup;   // 32
constexpr int kModelChunk = 4;
static_assert(kMaxDims <= kv::kMaxDims, "the model limit fits the lane split");

__global__ __launch_bounds__(kThreads) void svr_bank_kernel(SvrDev m, const double *__restrict__ feats, long long ld,
                                                            long long n_vec, double *__restrict__ out,
                                                            long long ld_out) {
    __shared__ double tile[kTile * kMaxDims];
    __shared__ double coef[kTile];
    const int tid = threadIdx.x, lane = tid % kGroupLanes, group = tid / kGroupLanes;
    const int M = (m.n_dims + kGroupLanes - 1) / kGroupLanes, pitch = M * kGroupLanes;
    const long long w0 = (long long)blockIdx.x * kWinPerBlock + group * kWinPerGroup;
    const int m_begin = blockIdx.y * kModelChunk, m_end = min(m.n_models, m_begin + kModelChunk);
    double x[kWinPerGroup][kMaxM];
    for (int mi = m_begin; mi < m_end; ++mi) {
        if (mi == m_begin || !m.same_prev[mi]) {          // this model's standardisation (workgroup-uniform branch)
            const double *mean = m.mean + (long long)mi * m.n_dims, *scale = m.scale + (long long)mi * m.n_dims;
#pragma unroll
            for (int w = 0; w < kWinPerGroup; ++w) {
#pragma unroll
                for (int i = 0; i < kMaxM; ++i) {
                    const int d = lane + kGroupLanes * i;
                    x[w][i] = (i < M && d < m.n_dims && w0 + w < n_vec) ? (feats[(long long)d * ld + w0 + w] - mean[d]) / scale[d] : 0.0;
                }
            }
        }
        const long long s_begin = m.sv_off[mi], s_end = m.sv_off[mi + 1];
        const bool rbf = m.rbf[mi] != 0;
        const double gamma = m.gamma[mi];
        double acc[kWinPerGroup] = {0.0, 0.0};
        for (long long base = s_begin; base < s_end; base += kTile) {
            __syncthreads();
            kv::stage_rows(tile, m.sv, base, s_end, m.n_dims, pitch, tid);
            if (tid < kTile) coef[tid] = base + tid < s_end ? m.coef[base + tid] : 0.0;
            __syncthreads();
            const int cnt = (int)min((long long)kTile, s_end - base);
            for (int j = 0; j < cnt; ++j) {
                const double *t = tile + j * pitch + lane;
                double p[kWinPerGroup] = {0.0, 0.0};
                if (rbf) {
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
                const double c = coef[j];
#pragma unroll
                for (int w = 0; w < kWinPerGroup; ++w) {
                    double kv = group_sum(p[w]);
                    if (rbf) kv = exp(-gamma * kv);
                    acc[w] = fma(c, kv, acc[w]);
                }
            }
        }
        if (lane == 0) {
            const double rho = m.rho[mi];
#pragma unroll
            for (int w = 0; w < kWinPerGroup; ++w)
                if (w0 + w < n_vec) out[(long long)mi * ld_out + w0 + w] = acc[w] - rho;
        }
    }
}

}  // namespace svr
}  // namespace paa
