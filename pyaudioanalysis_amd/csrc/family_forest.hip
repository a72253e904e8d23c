// Tree-ensemble classification (kernels_forest.hpp: audioTrainTest.classifier_wrapper for the "randomforest", "extratrees"
// and "gradientboosting" models) and the fit of the first two (kernels_treefit.hpp: audioTrainTest.train_random_forest /
// train_extra_trees and the forest half of evaluate_classifier) and of the forest regressor (train_random_forest_regression and
// the "randomforest" sweep of evaluate_regression) and of the third (kernels_boost.hpp and the kFriedman instance of
// tree_fit_kernel: train_gradient_boosting and the "gradientboosting" sweep) -- own translation unit, see model_launch.hpp.
#include <cstdlib>
#include <cstring>

#include "model_launch.hpp"
#include "kernels_forest.hpp"
#include "kernels_treefit.hpp"
#include "kernels_boost.hpp"

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

int tree_prep(const treefit::TreeDev &m, int n_jobs, int n_max, hipStream_t stream) {
    using namespace paa::treefit;
    if (n_jobs < 1 || n_jobs > 65535 || n_max < 1 || n_max > kMaxRows || m.n_dims < 1 || m.n_dims > kMaxDims) return -1;
    if (hipMemsetAsync(m.flags, 0, (size_t)n_jobs * sizeof(int), stream) != hipSuccess) return -1;
    const long long elems = (long long)n_max * m.n_dims;
    hipLaunchKernelGGL(tree_prep_kernel, dim3((unsigned)((elems + kThreads - 1) / kThreads), (unsigned)n_jobs), dim3(kThreads), 0,
                       stream, m);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The launch of tree_fit_kernel<SPLITTER, CRIT>.  configure: size the LDS for inbag_max (and k_max classes) and write the geometry into
// m; false: m holds it already.  LDS: the sort words (best: a power of two of 64-bit words; random: the partition's 32-bit buffer) |
// the rows | kGini under the best splitter: the class histogram, 256 columns (128 above 32 classes, which keeps the largest launch
// below the CU's 160 KB) | the feature arrays.  The regression criteria keep the chunk sums of the candidate scan in registers (one
// chunk per thread), so they have no histogram: 96.5 KB at 8192 rows.  The callers below instantiate tree_fit_kernel<kBest, kGini>,
// tree_fit_kernel<kRandom, kGini>, tree_fit_kernel<kBest, kMse> and tree_fit_kernel<kBest, kFriedman>
template <int SPLITTER, int CRIT>
static int tree_fit_launch(treefit::TreeDev &m, int n_tasks, int inbag_max, int k_max, hipStream_t stream, bool configure) {
    using namespace paa::treefit;
    if (configure) {
        int p2 = 2;
        while (p2 < inbag_max) p2 <<= 1;
        m.lds_keys = SPLITTER == kBest ? p2 : (inbag_max + 1) / 2;
        m.lds_rows = (inbag_max + 1) / 2 * 2;
        m.hist_cols = CRIT != kGini ? kThreads : k_max > 32 ? 128 : 256;
        const size_t hist = SPLITTER == kBest && CRIT == kGini ? (size_t)k_max * (m.hist_cols + 1) * sizeof(int) : 0;
        m.lds_feat = (int)((size_t)m.lds_keys * 8 + (size_t)m.lds_rows * 4 + hist);
    }
    const size_t lds = ((size_t)m.lds_feat + 2 * (size_t)m.n_dims * sizeof(unsigned short) + 7) / 8 * 8;
    if (lds > 152 * 1024 || m.lds_rows < inbag_max) return -2;
    if (configure && lds > 32 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void *>(&tree_fit_kernel<SPLITTER, CRIT>),
                                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return -1;
    hipLaunchKernelGGL((tree_fit_kernel<SPLITTER, CRIT>), dim3((unsigned)n_tasks), dim3(kThreads), lds, stream, m);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int tree_fit(treefit::TreeDev &m, int n_tasks, int splitter, int inbag_max, int k_max, hipStream_t stream) {
    using namespace paa::treefit;
    if (m.n_dims < 1 || m.n_dims > kMaxDims || inbag_max < 1 || inbag_max > kMaxRows || k_max < 1 || k_max > kMaxClasses) return -2;
    if (n_tasks < 1 || (splitter != kBest && splitter != kRandom)) return -1;
    return splitter == kBest ? tree_fit_launch<kBest, kGini>(m, n_tasks, inbag_max, k_max, stream, true)
                             : tree_fit_launch<kRandom, kGini>(m, n_tasks, inbag_max, k_max, stream, true);
}

int tree_fit_reg(treefit::TreeDev &m, int n_tasks, int inbag_max, hipStream_t stream) {
    using namespace paa::treefit;
    if (m.n_dims < 1 || m.n_dims > kMaxDims || inbag_max < 1 || inbag_max > kMaxRows) return -2;
    if (n_tasks < 1 || !m.target) return -1;
    return tree_fit_launch<kBest, kMse>(m, n_tasks, inbag_max, 1, stream, true);
}

int tree_fit_boost(treefit::TreeDev &m, int n_tasks, int inbag_max, hipStream_t stream, bool configure) {
    using namespace paa::treefit;
    if (m.n_dims < 1 || m.n_dims > kMaxDims || inbag_max < 1 || inbag_max > kMaxRows) return -2;
    if (n_tasks < 1 || !m.target || m.max_depth < 0 || (m.raw && (!m.boost || !m.label))) return -1;
    return tree_fit_launch<kBest, kFriedman>(m, n_tasks, inbag_max, 1, stream, configure);
}

int boost_gradient(const boost::BoostDev &m, int n_jobs, int stage, hipStream_t stream) {
    if (n_jobs < 1 || stage < 0) return -1;
    hipLaunchKernelGGL(boost::boost_gradient_kernel, dim3((unsigned)n_jobs), dim3(boost::kThreads), 0, stream, m, stage);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int tree_gather(const double *d_X, int n_dims, const int *d_rows, long long n_rows, double *d_out, long long ld, hipStream_t stream) {
    using namespace paa::treefit;
    if (n_rows < 1 || n_dims < 1 || ld < n_rows) return -1;
    const long long elems = n_rows * n_dims;
    hipLaunchKernelGGL(tree_gather_kernel, dim3((unsigned)((elems + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, d_X, n_dims,
                       d_rows, n_rows, d_out, ld);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

void tree_fit_geometry(int out6[6]) {
    out6[0] = treefit::kThreads;
    out6[1] = treefit::kMaxRows;
    out6[2] = treefit::kMaxClasses;
    out6[3] = treefit::kMaxDims;
    out6[4] = treefit::kMaxWeight;
    out6[5] = (int)(treefit::kChunkBytes >> 20);
}

}  // namespace launch
}  // namespace paa
