// Tree-ensemble classification (kernels_forest.hpp: audioTrainTest.classifier_wrapper for the "randomforest", "extratrees"
// and "gradientboosting" models) -- own translation unit, see model_launch.hpp.
#include <cstdlib>
#include <cstring>

#include "model_launch.hpp"
#include "kernels_forest.hpp"

namespace paa {
namespace launch {

int forest(const forest::ForestDev &m, const double *d_feats, long long ld, long long n_vec, const double *d_mean,
           const double *d_scale, int *d_leaves, int *d_label, double *d_raw, double *d_proba, hipStream_t stream) {
    using namespace paa::forest;
    if (m.n_trees < 1 || m.n_classes < 1 || m.n_classes > kMaxClasses || m.n_dims < 1 || m.n_dims > kMaxDims ||
        m.n_outputs < 1 || (m.boosted && m.n_trees % m.n_outputs) || n_vec < 1)
        return -1;
    const size_t lds = (size_t)m.n_dims * kWin * sizeof(float);
    for (long long c0 = 0; c0 < n_vec; c0 += kChunk) {
        const long long n = n_vec - c0 < kChunk ? n_vec - c0 : kChunk;
        const long long xblocks = (n + kWin - 1) / kWin;
        // trees per workgroup: a multiple of the 4 waves, doubled while at least 2048 workgroups remain (the staging of the
        // windows' vectors is then shared by more trees)
        int tpb = kTravWaves;
        while (tpb < m.n_trees && xblocks * ((m.n_trees + 2 * tpb - 1) / (2 * tpb)) >= 2048) tpb *= 2;
        const int yblocks = (m.n_trees + tpb - 1) / tpb;
        hipLaunchKernelGGL(forest_traverse_kernel, dim3((unsigned)xblocks, (unsigned)yblocks), dim3(kTravThreads), lds, stream, m,
                           d_feats + c0, ld, n, d_mean, d_scale, tpb, d_leaves);
        if (hipGetLastError() != hipSuccess) return -1;
        hipLaunchKernelGGL(forest_reduce_kernel, dim3((unsigned)((n + kReduceThreads - 1) / kReduceThreads)),
                           dim3(kReduceThreads), 0, stream, m, d_feats + c0, ld, n, d_mean, d_scale, d_leaves, d_label + c0,
                           d_raw + c0 * m.n_outputs, d_proba + c0 * m.n_classes);
        if (hipGetLastError() != hipSuccess) return -1;
    }
    return 0;
}

}  // namespace launch
}  // namespace paa
