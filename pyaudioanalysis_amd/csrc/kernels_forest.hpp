// Tree-ensemble classification over many feature vectors: what audioTrainTest.classifier_wrapper (audioTrainTest.py:84-93)
// asks scikit-learn for once per mid-term window (audioSegmentation.mid_term_file_classification, :586-591) or once per file
// (audioTrainTest.file_classification, :1091-1095) with a "randomforest", "extratrees" or "gradientboosting" model.
// The rules are scikit-learn's (1.4 and later), kept bit for bit:
//  * input: x = (feat - mean) / std in FP64, then rounded to float32 (scikit-learn validates X to float32 before a tree
//    walk); a split goes left when (double)x32[feature] <= threshold; a NaN goes the node's missing-value way
//    (kMissingLeft, _tree.pyx _apply_dense); a float32 infinity (|x| > FLT_MAX) is an error for every model and a NaN for
//    a boosted one: label -1 / -2, the host raises scikit-learn's ValueError;
//  * averaged forest: sum[c] = 0.0 + value_0[leaf_0][c] + value_1[leaf_1][c] + ... in tree order, proba = sum / n_trees,
//    label = first arg-max of proba (ForestClassifier.predict_proba with n_jobs=None);
//  * boosted: raw[k] = init[k], then per stage s raw[k] = raw[k] + (learning_rate * value[leaf]) with no FMA
//    (predict_stages); two classes: one output, label = raw >= 0, proba = (1 - expit, expit); more: label = first arg-max
//    of raw, proba = softmax with the maximum subtracted first.
// Two kernels per chunk of windows:
//  * forest_traverse_kernel: a workgroup owns kWin windows (one per lane) and a block of trees (one tree per wave at a
//    time); it stages the windows' float32 vectors in LDS as [dim][kWin] (lane w reads word d * 64 + w: bank w, conflict
//    free whatever the features), and every lane walks its window down the tree, one 16-byte node load per level, and
//    writes the leaf slot to leaves[tree][window];
//  * forest_reduce_kernel: one thread per window adds the leaf values in tree order (classes in register chunks of
//    kClassChunk), then takes the arg-max and the link.  The tree order of the sum is what makes it bit-identical, so no
//    tree-parallel reduction.
// The host (lib_forest.hpp) packs every tree in preorder, so a child's index is always greater than its parent's and a
// walk ends after at most the tree's node count; every index was validated before the upload.
#pragma once
#include "device_common.hpp"
#include "model_launch.hpp"

namespace paa {
namespace forest {

constexpr int kTravThreads = 256;                                   // 4 waves: 4 trees at a time
constexpr int kTravWaves = kTravThreads / kWave;
constexpr int kReduceThreads = 256;
constexpr int kClassChunk = 8;                                      // running sums kept in registers per pass

// one visited node = one 16-byte load
__device__ __forceinline__ Node load_node(const Node *nodes, int n) {
    const uint4 w = reinterpret_cast<const uint4 *>(nodes)[n];
    Node r;
    r.threshold = __hiloint2double((int)w.y, (int)w.x);
    r.meta = (int)w.z;
    r.next = (int)w.w;
    return r;
}

// scikit-learn's input: the FP64 standardisation, then the float32 cast of check_array(dtype=np.float32)
__device__ __forceinline__ float std32(double f, double mean, double scale) { return (float)((f - mean) / scale); }

__global__ __launch_bounds__(kTravThreads) void forest_traverse_kernel(ForestDev m, const double *__restrict__ feats,
                                                                       long long ld, long long n_vec,
                                                                       const double *__restrict__ mean,
                                                                       const double *__restrict__ scale, int trees_per_block,
                                                                       int *__restrict__ leaves) {
    extern __shared__ float xs[];                                   // [n_dims][kWin]
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const long long v0 = (long long)blockIdx.x * kWin;
    for (int i = tid; i < m.n_dims * kWin; i += kTravThreads) {
        const int d = i / kWin, w = i % kWin;
        const long long v = v0 + w;
        xs[i] = v < n_vec ? std32(feats[(long long)d * ld + v], mean[d], scale[d]) : 0.0f;
    }
    __syncthreads();
    const long long v = v0 + lane;
    if (v >= n_vec) return;
    const int t_end = min(m.n_trees, (int)(blockIdx.y + 1) * trees_per_block);
    for (int t = blockIdx.y * trees_per_block + wave; t < t_end; t += kTravWaves) {
        int n = m.roots[t];
        Node node = load_node(m.nodes, n);
        while (!(node.meta & kLeaf)) {
            const float x = xs[(node.meta & kFeatureMask) * kWin + lane];
            const bool left = x != x ? (node.meta & kMissingLeft) != 0 : (double)x <= node.threshold;
            n = left ? n + 1 : node.next;
            node = load_node(m.nodes, n);
        }
        leaves[(long long)t * n_vec + v] = node.next;
    }
}

#pragma clang fp contract(off)
__global__ __launch_bounds__(kReduceThreads) void forest_reduce_kernel(ForestDev m, const double *__restrict__ feats,
                                                                       long long ld, long long n_vec,
                                                                       const double *__restrict__ mean,
                                                                       const double *__restrict__ scale,
                                                                       const int *__restrict__ leaves, int *__restrict__ label,
                                                                       double *__restrict__ raw, double *__restrict__ proba) {
    const long long v = (long long)blockIdx.x * kReduceThreads + threadIdx.x;
    if (v >= n_vec) return;
    bool any_inf = false, any_nan = false;
    for (int d = 0; d < m.n_dims; ++d) {
        const float x = std32(feats[(long long)d * ld + v], mean[d], scale[d]);
        any_inf |= __builtin_isinf(x);
        any_nan |= x != x;
    }
    const int K = m.n_outputs;
    double *r = raw + v * K;
    for (int c0 = 0; c0 < K; c0 += kClassChunk) {
        double acc[kClassChunk];
#pragma unroll
        for (int j = 0; j < kClassChunk; ++j) acc[j] = (m.boosted && c0 + j < K) ? m.init[c0 + j] : 0.0;
        if (m.boosted) {
            const int stages = m.n_trees / K;
            for (int s = 0; s < stages; ++s) {
#pragma unroll
                for (int j = 0; j < kClassChunk; ++j) {
                    if (c0 + j < K) {
                        const int slot = leaves[(long long)(s * K + c0 + j) * n_vec + v];
                        const double step = m.learning_rate * m.leaf_values[slot];
                        acc[j] = acc[j] + step;
                    }
                }
            }
        } else {
            for (int t = 0; t < m.n_trees; ++t) {
                const double *row = m.leaf_values + (long long)leaves[(long long)t * n_vec + v] * K + c0;
#pragma unroll
                for (int j = 0; j < kClassChunk; ++j)
                    if (c0 + j < K) acc[j] += row[j];
            }
        }
#pragma unroll
        for (int j = 0; j < kClassChunk; ++j)
            if (c0 + j < K) r[c0 + j] = acc[j];
    }
    double *p = proba + v * m.n_classes;
    int best = 0;
    if (!m.boosted) {
        const double n = (double)m.n_trees;
        double top = r[0] / n;
        for (int c = 0; c < K; ++c) {
            const double q = r[c] / n;
            p[c] = q;
            if (q > top) { top = q; best = c; }
        }
    } else if (K == 1) {
        const double z = r[0];
        const double e = 1.0 / (1.0 + exp(-z));                     // expit
        p[0] = 1.0 - e;
        p[1] = e;
        best = z >= 0.0 ? 1 : 0;
    } else {
        double top = r[0];
        for (int c = 1; c < K; ++c)
            if (r[c] > top) { top = r[c]; best = c; }
        double sum = 0.0;
        for (int c = 0; c < K; ++c) {
            const double e = exp(r[c] - top);
            p[c] = e;
            sum += e;
        }
        for (int c = 0; c < K; ++c) p[c] = p[c] / sum;
    }
    label[v] = (m.boosted && any_nan) ? -2 : any_inf ? -1 : best;
}
#pragma clang fp contract(fast)

}  // namespace forest
}  // namespace paa
