// The multi-class probabilistic SVC (kernels_svc.hpp: audioTrainTest.classifier_wrapper for the shipped SVM models) -- own
// translation unit, see model_launch.hpp.
#include <cstdlib>
#include <cstring>

#include "model_launch.hpp"
#include "kernels_svc.hpp"

namespace paa {
namespace launch {

template <int K>
static int svc_proba(const svc::SvcDev &m, long long n_vec, const double *d_sums, int *d_label, double *d_proba,
                     hipStream_t stream) {
    constexpr int T = svc::proba_threads<K>();
    hipLaunchKernelGGL(svc::svc_proba_kernel<K>, dim3((unsigned)((n_vec + T - 1) / T)), dim3(T), 0, stream, m, n_vec, d_sums,
                       d_label, d_proba);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int svc(const svc::SvcDev &m, const double *d_feats, long long ld, long long n_vec, const double *d_mean, const double *d_scale,
        double *d_sums, int *d_label, double *d_proba, hipStream_t stream) {
    if (m.k < 2 || m.k > svc::kMaxClasses || m.n_dims < 1 || m.n_dims > svc::kMaxDims || n_vec < 1) return -1;
    const long long blocks = (n_vec + svc::kWinPerBlock - 1) / svc::kWinPerBlock;
    hipLaunchKernelGGL(svc::svc_class_sums_kernel, dim3((unsigned)blocks), dim3(svc::kThreads), 0, stream, m, d_feats, ld, n_vec,
                       d_mean, d_scale, d_sums);
    if (hipGetLastError() != hipSuccess) return -1;
    return dispatch_int<2, svc::kMaxClasses>(m.k, [&](auto K) { return svc_proba<K()>(m, n_vec, d_sums, d_label, d_proba, stream); });
}

}  // namespace launch
}  // namespace paa
