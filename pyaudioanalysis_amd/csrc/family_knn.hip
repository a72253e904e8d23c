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

template <int K>
static int knn_split_at(const knn::KnnSplitDev &m, long long n_blocks, int *d_label, double *d_proba, int *d_neighbors,
                        hipStream_t stream) {
    const int pitch = (m.n_dims + knn::kGroupLanes - 1) / knn::kGroupLanes * knn::kGroupLanes;
    const size_t lds = (size_t)knn::kTile * pitch * sizeof(double);
    hipLaunchKernelGGL(knn::knn_split_kernel<K>, dim3((unsigned)n_blocks), dim3(knn::kThreads), lds, stream, m, d_label, d_proba,
                       d_neighbors);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int knn_split_k_launch(int k_max) {
    for (int K : knn::kSplitKs)
        if (k_max >= 1 && k_max <= K) return K;
    return 0;
}

int knn_split(const knn::KnnSplitDev &m, long long n_blocks, int k_max, int *d_label, double *d_proba, int *d_neighbors,
              hipStream_t stream) {
    if (m.n_dims < 1 || m.n_dims > knn::kMaxDims || m.max_classes < 1 || m.max_classes > knn::kMaxClasses || n_blocks < 1 ||
        n_blocks > 0x7fffffffLL)
        return -1;
    switch (knn_split_k_launch(k_max)) {
    case 1: return knn_split_at<1>(m, n_blocks, d_label, d_proba, d_neighbors, stream);
    case 2: return knn_split_at<2>(m, n_blocks, d_label, d_proba, d_neighbors, stream);
    case 4: return knn_split_at<4>(m, n_blocks, d_label, d_proba, d_neighbors, stream);
    case 8: return knn_split_at<8>(m, n_blocks, d_label, d_proba, d_neighbors, stream);
    case 16: return knn_split_at<16>(m, n_blocks, d_label, d_proba, d_neighbors, stream);
    case 32: return knn_split_at<32>(m, n_blocks, d_label, d_proba, d_neighbors, stream);
    }
    return -1;
}

void knn_split_geometry(int out10[10]) {
    out10[0] = knn::kQueriesPerBlock;
    out10[1] = knn::kTile;
    out10[2] = knn::kGroupLanes;
    out10[3] = (int)(sizeof(knn::kSplitKs) / sizeof(knn::kSplitKs[0]));
    for (int i = 0; i < 6; ++i) out10[4 + i] = knn::kSplitKs[i];
}

}  // namespace launch
}  // namespace paa
