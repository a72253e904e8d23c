// k-nearest-neighbour classification (kernels_knn.hpp: audioTrainTest.Knn.classify for the shipped knn_* models) -- own
// translation unit, see model_launch.hpp.
#include <cstdlib>
#include <cstring>

#include "model_launch.hpp"
#include "kernels_knn.hpp"

namespace paa {
namespace launch {

template <int K>
static int knn_at(const knn::KnnDev &m, const double *d_feats, long long ld, long long n_vec, const double *d_mean,
                  const double *d_scale, int *d_label, double *d_proba, int *d_neighbors, hipStream_t stream) {
    const long long blocks = (n_vec + knn::kQueriesPerBlock - 1) / knn::kQueriesPerBlock;
    const int pitch = (m.n_dims + knn::kGroupLanes - 1) / knn::kGroupLanes * knn::kGroupLanes;
    const size_t lds = (size_t)knn::kTile * pitch * sizeof(double);
    hipLaunchKernelGGL(knn::knn_kernel<K>, dim3((unsigned)blocks), dim3(knn::kThreads), lds, stream, m, d_feats, ld, n_vec,
                       d_mean, d_scale, d_label, d_proba, d_neighbors);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int knn(const knn::KnnDev &m, const double *d_feats, long long ld, long long n_vec, const double *d_mean, const double *d_scale,
        int *d_label, double *d_proba, int *d_neighbors, hipStream_t stream) {
    if (m.k < 1 || m.k > knn::kMaxK || m.n_classes < 1 || m.n_classes > knn::kMaxClasses || m.n_dims < 1 ||
        m.n_dims > knn::kMaxDims || m.n_train < 1 || n_vec < 1)
        return -1;
    return dispatch_int<1, knn::kMaxK>(m.k, [&](auto K) {
        return knn_at<K()>(m, d_feats, ld, n_vec, d_mean, d_scale, d_label, d_proba, d_neighbors, stream);
    });
}

}  // namespace launch
}  // namespace paa
