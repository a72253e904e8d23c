// Gaussian HMM segmentation (kernels_hmm.hpp: emission log-likelihoods, Viterbi by segments, training statistics) -- own
// translation unit, see model_launch.hpp.
#include <cstdlib>
#include <cstring>

#include "model_launch.hpp"
#include "kernels_hmm.hpp"

namespace paa {
namespace launch {

static bool hmm_ok(const hmm::HmmDev &m) {
    return m.n_states >= 1 && m.n_states <= hmm::kMaxStates && m.n_dims >= 1 && m.n_dims <= hmm::kMaxDims && m.kp >= 2 &&
           m.kp <= hmm::kMaxStates && (m.kp & (m.kp - 1)) == 0 && m.kp >= m.n_states;
}

template <int KP>
static int hmm_emission_at(const hmm::HmmDev &m, const double *d_feats, long long ld, long long n_vec, double *d_loglik,
                           hipStream_t stream) {
    if (m.kp != KP) {
        if constexpr (KP < hmm::kMaxStates) return hmm_emission_at<KP * 2>(m, d_feats, ld, n_vec, d_loglik, stream);
        return -1;
    }
    const long long blocks = (n_vec + hmm::kEmitThreads - 1) / hmm::kEmitThreads;
    hipLaunchKernelGGL(hmm::emission_kernel<KP>, dim3((unsigned)blocks), dim3(hmm::kEmitThreads), 0, stream, m, d_feats, ld,
                       n_vec, d_loglik);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int hmm_emission(const hmm::HmmDev &m, const double *d_feats, long long ld, long long n_vec, double *d_loglik, hipStream_t stream) {
    if (!hmm_ok(m) || n_vec < 1 || n_vec > 0x7fffffffLL) return -1;
    return hmm_emission_at<2>(m, d_feats, ld, n_vec, d_loglik, stream);
}

template <int KP>
static int hmm_decode_at(const hmm::HmmDev &m, const double *d_loglik, const hmm::Segment *d_segs, long long n_seg,
                         const long long *d_seq_seg, long long n_seq, int multi, double *d_M, double *d_V, double *d_Vout,
                         unsigned char *d_psi, unsigned char *d_emap, int *d_seg_end, int *d_states, double *d_logprob,
                         hipStream_t stream) {
    if (m.kp != KP) {
        if constexpr (KP < hmm::kMaxStates)
            return hmm_decode_at<KP * 2>(m, d_loglik, d_segs, n_seg, d_seq_seg, n_seq, multi, d_M, d_V, d_Vout, d_psi, d_emap,
                                         d_seg_end, d_states, d_logprob, stream);
        return -1;
    }
    constexpr int G = 64 / KP;
    if (multi) {
        const long long tasks = n_seg * m.n_states;
        hipLaunchKernelGGL(hmm::product_kernel<KP>, dim3((unsigned)((tasks + G - 1) / G)), dim3(64), 0, stream, m, d_loglik,
                           d_segs, n_seg, d_M);
        hipLaunchKernelGGL(hmm::chain_kernel<KP>, dim3((unsigned)((n_seq + G - 1) / G)), dim3(64), 0, stream, m, d_loglik,
                           d_segs, d_seq_seg, n_seq, (const double *)d_M, d_V);
    }
    hipLaunchKernelGGL(hmm::segment_kernel<KP>, dim3((unsigned)((n_seg + G - 1) / G)), dim3(64), 0, stream, m, d_loglik, d_segs,
                       n_seg, (const double *)d_V, d_Vout, d_psi, d_emap);
    hipLaunchKernelGGL(hmm::pick_kernel, dim3((unsigned)n_seq), dim3(64), 0, stream, m.n_states, KP, d_seq_seg,
                       (const double *)d_Vout, (const unsigned char *)d_emap, d_seg_end, d_logprob);
    hipLaunchKernelGGL(hmm::gather_kernel, dim3((unsigned)n_seg), dim3(64), 0, stream, KP, d_segs, (const int *)d_seg_end,
                       (const unsigned char *)d_psi, d_states);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int hmm_decode(const hmm::HmmDev &m, const double *d_loglik, const hmm::Segment *d_segs, long long n_seg,
               const long long *d_seq_seg, long long n_seq, int multi, double *d_M, double *d_V, double *d_Vout,
               unsigned char *d_psi, unsigned char *d_emap, int *d_seg_end, int *d_states, double *d_logprob, hipStream_t stream) {
    if (!hmm_ok(m) || n_seg < 1 || n_seq < 1 || n_seq > n_seg || n_seg * m.n_states > 0x7fffffffLL) return -1;
    return hmm_decode_at<2>(m, d_loglik, d_segs, n_seg, d_seq_seg, n_seq, multi, d_M, d_V, d_Vout, d_psi, d_emap, d_seg_end,
                            d_states, d_logprob, stream);
}

int hmm_stats(const double *d_feats, long long ld, long long n_vec, const int *d_labels, int n_states, int n_dims,
              int *d_counts, double *d_means, double *d_stds, hipStream_t stream) {
    if (n_states < 1 || n_states > hmm::kMaxStates || n_dims < 1 || n_dims > hmm::kMaxDims || n_vec < 1) return -1;
    const long long want = (n_vec + hmm::kStatThreads - 1) / hmm::kStatThreads;
    hipLaunchKernelGGL(hmm::stats_count_kernel, dim3((unsigned)(want < 64 ? want : 64)), dim3(hmm::kStatThreads), 0, stream,
                       d_labels, n_vec, n_states, d_counts);
    hipLaunchKernelGGL(hmm::stats_moment_kernel, dim3((unsigned)(n_states * n_dims)), dim3(hmm::kStatThreads), 0, stream, d_feats,
                       ld, n_vec, d_labels, n_states, (const int *)d_counts, d_means, d_stds, n_dims);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace launch
}  // namespace paa
