// Fitting the trees of audioTrainTest.train_random_forest / train_extra_trees (audioTrainTest.py:158-178, :202-219; the sweep of
// evaluate_classifier :631-700): scikit-learn 1.7.2's DepthFirstTreeBuilder with the Gini criterion, the BestSplitter
// ("randomforest") or the RandomSplitter ("extratrees"), max_features = max(1, int(sqrt(n_dims))), min_samples_split = 2,
// min_samples_leaf = 1, no depth limit, no missing values, integer sample weights (a forest's bootstrap counts; 0: out of the
// bag) -- restated operation for operation (sklearn/tree/_tree.pyx, _splitter.pyx, _partitioner.pyx, _criterion.pyx,
// _utils.pyx, utils/_random.pxd), so that every array of the tree equals scikit-learn's bit for bit:
//  * input x32 = (float)((x - mean) / scale), FP64 first (kernels_forest.hpp has the same rule), one feature-major copy per
//    job made by tree_prep_kernel and shared by the job's trees;
//  * our_rand_r: 32-bit xorshift 13 / 17 / 5, seed 0 replaced by 1, the result modulo 2^31; rand_int = low + r % (high - low);
//    rand_uniform = (high - low) * r / 2147483647.0 + low in FP64;
//  * the Fisher-Yates feature draw of node_split_best / node_split_random with its drawn, known and found constant counts;
//    `features` persists over the nodes of a tree; `constant_features` is ONE array whose first n_known entries belong to the
//    node being split (a child only writes behind its parent's entries, so the depth-first order keeps every prefix intact);
//  * FEATURE_THRESHOLD is ZERO: _partitioner.pxd declares `cdef float32_t FEATURE_THRESHOLD = 1e-7`, but the initialiser of a
//    cdef variable in a .pxd takes no effect, and the compiled 1.7.2 compares against 0 (measured: it splits two adjacent float32
//    values, 7.5e-9 apart at 0.1, with either splitter).  So a feature is constant in a node when max <= min;
//  * best splitter: the node's (value, row) pairs are sorted in LDS (bitonic, 64-bit words: ties fall in any order, nothing
//    depends on it); the candidates are the positions p with v[p] > v[p - 1]; the proxy improvement is
//    -w_right * gini_right - w_left * gini_left with gini = 1 - sum_k count_k^2 / (w * w) in class order (Criterion.
//    proxy_impurity_improvement over Gini.children_impurity), the first strict maximum wins; the threshold is
//    v[p - 1] / 2.0 + v[p] / 2.0 in FP64, v[p - 1] when that equals v[p] or is infinite;
//  * random splitter: threshold = rand_uniform(min, max), min when it equals max; a row goes left when (double)x32 <= threshold;
//  * a node is a leaf when it has fewer than 2 rows, its impurity is <= DBL_EPSILON, no split was found (pos >= end) or the
//    split's improvement + DBL_EPSILON < 0 (min_impurity_decrease = 0);
//  * nodes are numbered in the order of popping: preorder, the left subtree first; value = counts / weighted count.
// Nothing depends on the order of the rows inside a node: the class statistics are sums of integer weights (LDS integer
// atomics), exact in FP64.  No FMA contraction anywhere scikit-learn's x86-64 build has none.
// One workgroup per tree.  A row of a tree is one 32-bit word (weight << 19 | class << 13 | place in the job's list); the rows,
// the sort words, the per-column class histograms of the candidate scan, the two feature arrays and the control block live in
// LDS; the stack of pending right children (its depth can reach the number of in-bag rows) and the outputs in global memory.
// Thread 0 runs the builder's control flow (the draws, the bookkeeping, the node records) and publishes what the others need
// through the control block; the data-parallel steps (class totals, gather, sort, scan, min / max, partition) use all threads.
//
// K19, the regressor (audioTrainTest.train_random_forest_regression and the "randomforest" sweep of evaluate_regression,
// audioTrainTest.py:229-233, :774-855): CRIT = kMse restates RegressionCriterion / MSE of _criterion.pyx over the BestSplitter
// with RandomForestRegressor's settings: max_features = n_dims (the draw loop ends when every non-constant feature was visited),
// one output.  The row word's class field is 0; the targets are a per-job double list in global memory, read through the row
// index of the word (sort words + row words + targets would fill the CU's 160 KB at 8192 rows, so they are not staged in LDS).
//  * per node sum_total = sum w y, sq_sum_total = sum (w y) y, weighted_n = sum w; value = sum_total / weighted_n; the root's
//    impurity is sq_sum_total / weighted_n - (sum_total / weighted_n)^2 (the square a plain product);
//  * the proxy at position p of the sorted rows is sum_left sum_left / w_left + sum_right sum_right / w_right with sum_left the
//    prefix of w y and sum_right = sum_total - sum_left; the first strict maximum wins;
//  * after the final partition sq_sum_left = sum_left (w y) y, sq_sum_right = sq_sum_total - sq_sum_left, and each child's
//    impurity is sq_sum / w - (sum / w)^2; improvement and the leaf rules are the classifier's.
// THE ORDER OF EVERY FLOATING-POINT SUM IS FIXED and depends only on the node's rows and the sorted order; there is no float atomic:
//  * a node's totals and the left child's sums: the node's rows (in the order the stable partitions left them) are cut into 256
//    consecutive chunks of ceil(n / 256) rows; thread t adds chunk t serially from 0.0 in row order; the 256 partial sums are
//    added by a xor butterfly within each wave (offsets 32, 16, .. 1) and the four wave sums as ((s0 + s1) + s2) + s3;
//  * the prefix of w y left of a candidate: the sorted rows (64-bit sort words: value, then weight, then the row's place) are cut
//    into the same 256 chunks; thread t adds chunk t serially; the chunk sums get an inclusive Hillis-Steele scan within each wave
//    (offsets 1, 2, .. 32), a chunk's exclusive prefix is (sum of the earlier waves' totals, in wave order from 0.0) + (the scan
//    value of the lane before, 0.0 for lane 0); from there thread t walks its chunk serially.
// So a tree is bit-identical run to run, alone or anywhere in a batch.  When the targets and weights make every such sum exact
// in FP64 (e.g. multiples of 2^-3, |y| <= 2^10, total weight <= 2^13: sum w y y needs 13 + 20 + 6 bits), the order is immaterial
// and every array equals scikit-learn's bit for bit; otherwise the sums may differ from scikit-learn's (which follow its introsort
// and in-place partition) in the last places, and a tie that rounding breaks may fall the other way: a valid CART tree, not
// scikit-learn's bits.
//
// K20, a boosting stage's tree (audioTrainTest.train_gradient_boosting and the "gradientboosting" sweep of evaluate_classifier,
// audioTrainTest.py:181-199, :631-700): CRIT = kFriedman restates FriedmanMSE over MSE for GradientBoostingClassifier's
// DecisionTreeRegressor(criterion="friedman_mse", max_depth = 3, max_features = None): the sums, the node value and every impurity are
// kMse's, in kMse's fixed order; compile-time differences only:
//  * the proxy at a candidate is diff diff / (w_left w_right) with diff = w_right sum_left - w_left sum_right, and the improvement
//    of the chosen split diff diff / (w_left w_right weighted_n_node_samples) (never negative, so it closes no node);
//  * a node is also a leaf when depth >= max_depth (the root has depth 0); the depth of a pending right child rides in the upper half of
//    its stack record's parent word (a node id is below 2^15);
//  * the leaf step (the sweep: TreeDev.raw and .boost set).  The targets of tree (job, class k) are the negative gradients r of that
//    class at the start of the stage (kernels_boost.hpp), read per job row as kMse reads them.  When the builder closes a leaf, over
//    the leaf's contiguous rows: num = (sum r) / n -- the node's sum_total, already formed in the fixed order -- times (K - 1) / K
//    (one double, 1.0 for two classes); den = (sum p (1 - p)) / n with p = (y == k) - r, chunk-serial then the fixed-shape sum; value =
//    0.0 when |den| < 1e-150, else num / den (_update_terminal_regions through np.average and _safe_divide); it replaces the leaf's
//    mean, internal nodes keep theirs.  Then raw[row] += learning_rate * value for the leaf's rows: a row lies in exactly one leaf of
//    the tree and the residuals were taken before the launch, so the update is in place and free of races.
// The Gini and MSE instances keep their operations.
#pragma once
#include "device_common.hpp"
#include "model_launch.hpp"

namespace paa {
namespace treefit {

constexpr int kRowBits = 13, kClassBits = 6;                       // kMaxRows = 2^13, kMaxClasses = 2^6, kMaxWeight = 2^13 - 1
constexpr float kFeatureThreshold = 0.0f;                          // FEATURE_THRESHOLD as the compiled scikit-learn 1.7.2 has it (see above)

__device__ __forceinline__ unsigned row_word(int weight, int cls, int row) {
    return ((unsigned)weight << (kRowBits + kClassBits)) | ((unsigned)cls << kRowBits) | (unsigned)row;
}
__device__ __forceinline__ int word_row(unsigned w) { return (int)(w & ((1u << kRowBits) - 1)); }
__device__ __forceinline__ int word_class(unsigned w) { return (int)((w >> kRowBits) & ((1u << kClassBits) - 1)); }
__device__ __forceinline__ int word_weight(unsigned w) { return (int)(w >> (kRowBits + kClassBits)); }

// a float as an unsigned key of the same order, and back
__device__ __forceinline__ unsigned key_of(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// scikit-learn's float32 input (kernels_forest.hpp: std32)
__device__ __forceinline__ float standardize32(double f, double mean, double scale) { return (float)((f - mean) / scale); }

__global__ __launch_bounds__(kThreads) void tree_prep_kernel(TreeDev m) {
    const TreeJob job = m.jobs[blockIdx.y];
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;          // element (row i, dim d) of the job, d fastest
    if (e >= (long long)job.n * m.n_dims) return;
    const int i = (int)(e / m.n_dims), d = (int)(e % m.n_dims);
    const float x = standardize32(m.X[(long long)m.idx[job.off + i] * m.n_dims + d], m.mean[(long long)job.stat * m.n_dims + d],
                                  m.scale[(long long)job.stat * m.n_dims + d]);
    m.x32[job.x_off + (long long)d * job.n + i] = x;
    if (x != x) atomicOr(&m.flags[blockIdx.y], 2);
    else if (__builtin_isinf(x)) atomicOr(&m.flags[blockIdx.y], 1);
}

__global__ __launch_bounds__(kThreads) void tree_gather_kernel(const double *__restrict__ X, int n_dims, const int *__restrict__ rows,
                                                               long long n_rows, double *__restrict__ out, long long ld) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n_rows * n_dims) return;
    const long long q = e / n_dims;
    const int d = (int)(e % n_dims);
    out[(long long)d * ld + q] = X[(long long)rows[q] * n_dims + d];
}

#pragma clang fp contract(off)

// utils/_random.pxd: our_rand_r
__device__ __forceinline__ unsigned rand_r(unsigned &s) {
    if (s == 0) s = 1;
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return s & 0x7fffffffu;                                         // % (RAND_R_MAX + 1)
}

// Gini.node_impurity / children_impurity of one side: the class counts in class order
__device__ __forceinline__ double gini_of(const int *counts, int pitch, int K, double w) {
    double sq = 0.0;
    for (int c = 0; c < K; ++c) {
        const double ck = (double)counts[c * pitch];
        sq = sq + ck * ck;
    }
    return 1.0 - sq / (w * w);
}

// the control block: written by thread 0 between two barriers, read by everyone after the second
struct Control {
    int start, end, parent, is_left, n_known, node, leaf, done;
    int w_node, cur_f, n_found, best_f, n_left;
    int closed;                                                     // (Friedman) the node just recorded is a leaf: read behind the loop's last barrier
    double best_thr, thr;
};

// exclusive prefix sum of v over the workgroup's threads and the total; s_w [4] is LDS
__device__ __forceinline__ int block_scan_excl(int v, int *s_w, int &total) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    int inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int u = __shfl_up(inc, o, kWave);
        if (lane >= o) inc += u;
    }
    if (lane == kWave - 1) s_w[wave] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kThreads / kWave; ++i) {
        const int t = s_w[i];
        if (i < wave) base += t;
        total += t;
    }
    __syncthreads();
    return base + inc - v;
}

// best splitter: the first strict maximum of the columns' (proxy, position) in position order; thread 0 keeps it when it beats the
// best of the features before, with the threshold between the two sorted values
__device__ __forceinline__ void best_of_columns(double bv, int bp, double *red_v, int *red_p, const unsigned long long *keys, int f,
                                                double &best_proxy, int &best_f, double &best_thr) {
    const int tid = threadIdx.x;
    red_v[tid] = bv;
    red_p[tid] = bp;
    __syncthreads();
    if (tid < kWave) {
        bv = red_v[4 * tid];
        bp = red_p[4 * tid];
#pragma unroll
        for (int q = 1; q < 4; ++q)
            if (red_v[4 * tid + q] > bv) {
                bv = red_v[4 * tid + q];
                bp = red_p[4 * tid + q];
            }
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const double ov = __shfl_down(bv, o, kWave);
            const int op = __shfl_down(bp, o, kWave);
            if (tid + o < kWave && ov > bv) {
                bv = ov;
                bp = op;
            }
        }
        if (tid == 0 && bv > best_proxy) {
            best_proxy = bv;
            best_f = f;
            const double v0 = (double)value_of((unsigned)(keys[bp - 1] >> 32)), v1 = (double)value_of((unsigned)(keys[bp] >> 32));
            best_thr = v0 / 2.0 + v1 / 2.0;
            if (best_thr == v1 || best_thr == INFINITY || best_thr == -INFINITY) best_thr = v0;
        }
    }
}

// (MSE) the sums of a, b and c over the workgroup's threads, in every thread: a xor butterfly within each wave, then the waves in order
__device__ __forceinline__ void block_sum3(double &a, double &b, double &c) {
    __shared__ double s_d[3][kThreads / kWave];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        a = a + __shfl_xor(a, o, kWave);
        b = b + __shfl_xor(b, o, kWave);
        c = c + __shfl_xor(c, o, kWave);
    }
    if (lane == 0) {
        s_d[0][wave] = a;
        s_d[1][wave] = b;
        s_d[2][wave] = c;
    }
    __syncthreads();
    a = ((s_d[0][0] + s_d[0][1]) + s_d[0][2]) + s_d[0][3];
    b = ((s_d[1][0] + s_d[1][1]) + s_d[1][2]) + s_d[1][3];
    c = ((s_d[2][0] + s_d[2][1]) + s_d[2][2]) + s_d[2][3];
    __syncthreads();
}

// (MSE) exclusive prefix of (v, w) over the workgroup's threads: Hillis-Steele within each wave, the earlier waves' totals in order
__device__ __forceinline__ void block_scan_excl_d(double v, int w, double &ev, int &ew) {
    __shared__ double s_v[kThreads / kWave];
    __shared__ int s_n[kThreads / kWave];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    double inc = v;
    int winc = w;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const double u = __shfl_up(inc, o, kWave);
        const int uw = __shfl_up(winc, o, kWave);
        if (lane >= o) {
            inc = u + inc;
            winc += uw;
        }
    }
    if (lane == kWave - 1) {
        s_v[wave] = inc;
        s_n[wave] = winc;
    }
    const double before = __shfl_up(inc, 1, kWave);
    __syncthreads();
    double base = 0.0;
    int wbase = 0;
#pragma unroll
    for (int i = 0; i < kThreads / kWave - 1; ++i)
        if (i < wave) {
            base = base + s_v[i];
            wbase += s_n[i];
        }
    __syncthreads();
    ev = base + (lane ? before : 0.0);
    ew = wbase + winc - w;
}

template <int SPLITTER, int CRIT>
__global__ __launch_bounds__(kThreads) void tree_fit_kernel(TreeDev m) {
    static_assert(CRIT == kGini || SPLITTER == kBest, "the regression criteria are built for the best splitter");
    constexpr bool kReg = CRIT != kGini;                            // real targets: the squared-error sums
    constexpr bool kFried = CRIT == kFriedman;                      // ... with Friedman's proxy and improvement, a depth limit, the leaf step
    extern __shared__ unsigned long long dyn[];
    __shared__ Control ctl;
    __shared__ int tot[kMaxClasses], left[kMaxClasses], s_w[kThreads / kWave], red_p[kThreads];
    __shared__ double red_v[kThreads];
    __shared__ float s_lo[kThreads / kWave], s_hi[kThreads / kWave];
    unsigned long long *keys = dyn;                                 // [lds_keys]: the sort words; the partition's buffer
    unsigned *rows = reinterpret_cast<unsigned *>(keys + m.lds_keys);       // [lds_rows]: the tree's rows, node after node
    int *hist = reinterpret_cast<int *>(rows + m.lds_rows);         // best splitter: [k][hist_cols + 1] class counts per column
    const int pitch = m.hist_cols + 1;
    const int tid = threadIdx.x;
    const TreeTask task = m.tasks[blockIdx.x];
    const TreeJob job = m.jobs[task.job];
    const int n = job.n, K = job.k, n_dims = m.n_dims;
    unsigned short *feat = reinterpret_cast<unsigned short *>(reinterpret_cast<char *>(dyn) + m.lds_feat);     // behind the histogram
    unsigned short *cons = feat + n_dims;
    const float *xj = m.x32 + job.x_off;
    const int *lab = CRIT == kGini || (kFried && m.label) ? m.label + job.off : nullptr;
    const double *tgt = !kReg ? nullptr : (kFried && m.boost) ? m.target + m.boost[blockIdx.x].off : m.target + job.off;
    const int *wt = task.w_off < 0 ? nullptr : m.weight + task.w_off;

    // the rows in the bag, in list order
    int n_bag;
    {
        const int chunk = (n + kThreads - 1) / kThreads, c0 = min(n, tid * chunk), c1 = min(n, c0 + chunk);
        int cnt = 0;
        for (int i = c0; i < c1; ++i) cnt += (wt ? wt[i] : 1) != 0;
        int at = block_scan_excl(cnt, s_w, n_bag);
        for (int i = c0; i < c1; ++i) {
            const int w = wt ? wt[i] : 1;
            if (w != 0) rows[at++] = row_word(w, CRIT == kGini ? lab[i] : 0, i);
        }
    }
    for (int d = tid; d < n_dims; d += kThreads) {
        feat[d] = (unsigned short)d;
        cons[d] = 0;
    }
    // thread 0's builder state
    unsigned rng = task.seed;
    int sp = 0, first = 1, depth = 0;
    double impurity = 0.0, w_total = 0.0;
    StackRec *stack = m.stack + task.node_off;
    if (tid == 0) {
        ctl.start = 0;
        ctl.end = n_bag;
        ctl.parent = -1;
        ctl.is_left = 0;
        ctl.n_known = 0;
        ctl.node = 0;
        ctl.done = 0;
    }
    __syncthreads();

    for (;;) {
        const int start = ctl.start, end = ctl.end, n_node = end - start, n_known = ctl.n_known, node = ctl.node;
        double sum_tot = 0.0, sq_tot = 0.0;                         // (MSE) the node's sum w y and sum (w y) y, in every thread
        if constexpr (CRIT == kGini) {
            // the class totals of the node
            if (tid < K) tot[tid] = 0;
            __syncthreads();
            for (int i = start + tid; i < end; i += kThreads) atomicAdd(&tot[word_class(rows[i])], word_weight(rows[i]));
            __syncthreads();
            if (tid == 0) {
                int w = 0;
                for (int c = 0; c < K; ++c) w += tot[c];
                if (first) {
                    impurity = gini_of(tot, 1, K, (double)w);
                    w_total = (double)w;
                    first = 0;
                }
                ctl.w_node = w;
                ctl.leaf = n_node < 2 || impurity <= DBL_EPSILON;
            }
            __syncthreads();
        } else {
            // RegressionCriterion.init: the node's totals, chunk-serial then the fixed-shape sum (see the header)
            const int chunk = (n_node + kThreads - 1) / kThreads, c0 = min(n_node, tid * chunk), c1 = min(n_node, c0 + chunk);
            double wn = 0.0;
            for (int i = c0; i < c1; ++i) {
                const unsigned w = rows[start + i];
                const double y = tgt[word_row(w)], wy = (double)word_weight(w) * y;
                sum_tot = sum_tot + wy;
                sq_tot = sq_tot + wy * y;
                wn = wn + (double)word_weight(w);                   // (integers below 2^26: exact)
            }
            block_sum3(sum_tot, sq_tot, wn);
            if (tid == 0) {
                if (first) {
                    impurity = sq_tot / wn - (sum_tot / wn) * (sum_tot / wn);
                    w_total = wn;
                    first = 0;
                }
                ctl.w_node = (int)wn;
                ctl.leaf = n_node < 2 || impurity <= DBL_EPSILON;
                if constexpr (kFried) ctl.leaf = ctl.leaf || depth >= m.max_depth;
            }
            __syncthreads();
        }
        const int w_node = ctl.w_node;
        if constexpr (CRIT == kGini) {
            if (tid < K) m.value[task.val_off + (long long)node * K + tid] = (double)tot[tid] / (double)w_node;
        } else {
            if (tid == 0) m.value[task.val_off + node] = sum_tot / (double)w_node;
        }

        // thread 0's split search state (Splitter.node_split)
        int f_i = n_dims, n_found = 0, n_drawn = 0, n_total = n_known, n_visited = 0, f_j = 0, best_f = -1;
        double best_proxy = -INFINITY, best_thr = 0.0, imp_l = 0.0, imp_r = 0.0;
        int leaf = ctl.leaf, n_left = 0;
        if (!leaf) {
            for (;;) {
                if (tid == 0) {                                     // the next feature to evaluate, or none
                    int f = -1;
                    while (f_i > n_total && (n_visited < m.max_features || n_visited <= n_found + n_drawn)) {
                        ++n_visited;
                        f_j = n_drawn + (int)(rand_r(rng) % (unsigned)(f_i - n_found - n_drawn));
                        if (f_j < n_known) {                        // a known constant: drawn, not evaluated
                            const unsigned short a = feat[n_drawn];
                            feat[n_drawn] = feat[f_j];
                            feat[f_j] = a;
                            ++n_drawn;
                            continue;
                        }
                        f_j += n_found;
                        f = feat[f_j];
                        break;
                    }
                    ctl.cur_f = f;
                    ctl.n_found = n_found;
                    ctl.best_f = best_f;
                    ctl.best_thr = best_thr;
                }
                __syncthreads();
                const int f = ctl.cur_f;
                if (f < 0) break;
                const float *xf = xj + (long long)f * n;
                bool constant;
                if constexpr (SPLITTER == kBest) {
                    int P2 = 2;
                    while (P2 < n_node) P2 <<= 1;
                    for (int i = tid; i < P2; i += kThreads) {
                        const unsigned w = i < n_node ? rows[start + i] : 0u;
                        keys[i] = i < n_node ? ((unsigned long long)key_of(xf[word_row(w)]) << 32) | w : ~0ull;
                    }
                    __syncthreads();
                    for (int k = 2; k <= P2; k <<= 1)
                        for (int j = k >> 1; j > 0; j >>= 1) {
                            for (int i = tid; i < P2 / 2; i += kThreads) {
                                const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a | j;
                                const unsigned long long ka = keys[a], kb = keys[b];
                                if ((ka > kb) == ((a & k) == 0)) {
                                    keys[a] = kb;
                                    keys[b] = ka;
                                }
                            }
                            __syncthreads();
                        }
                    constant = value_of((unsigned)(keys[n_node - 1] >> 32)) <= value_of((unsigned)(keys[0] >> 32)) + kFeatureThreshold;
                } else {
                    float lo = INFINITY, hi = -INFINITY;
                    for (int i = start + tid; i < end; i += kThreads) {
                        const float v = xf[word_row(rows[i])];
                        lo = fminf(lo, v);
                        hi = fmaxf(hi, v);
                    }
#pragma unroll
                    for (int o = kWave / 2; o > 0; o >>= 1) {
                        lo = fminf(lo, __shfl_xor(lo, o, kWave));
                        hi = fmaxf(hi, __shfl_xor(hi, o, kWave));
                    }
                    if (tid % kWave == 0) {
                        s_lo[tid / kWave] = lo;
                        s_hi[tid / kWave] = hi;
                    }
                    if (tid < K) left[tid] = 0;
                    __syncthreads();
                    lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
                    hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
                    constant = hi <= lo + kFeatureThreshold;
                    if (tid == 0 && !constant) {                    // rand_uniform(min, max)
                        double thr = ((double)hi - (double)lo) * (double)rand_r(rng) / 2147483647.0 + (double)lo;
                        if (thr == (double)hi) thr = (double)lo;
                        ctl.thr = thr;
                        ctl.n_left = 0;
                    }
                }
                if (tid == 0) {
                    if (constant) {                                 // found constant: behind the known ones
                        const unsigned short a = feat[f_j];
                        feat[f_j] = feat[n_total];
                        feat[n_total] = a;
                        ++n_found;
                        ++n_total;
                    } else {
                        --f_i;
                        const unsigned short a = feat[f_i];
                        feat[f_i] = feat[f_j];
                        feat[f_j] = a;
                    }
                }
                if (constant) {
                    __syncthreads();                                // (the control block is rewritten next)
                    continue;
                }
                if constexpr (SPLITTER == kBest && kReg) {
                    // sum w y and the weight left of every candidate: per chunk of consecutive sorted rows, a prefix over the chunks,
                    // then every thread walks its own chunk (see the header for the order)
                    const int chunk = (n_node + kThreads - 1) / kThreads, c0 = min(n_node, tid * chunk), c1 = min(n_node, c0 + chunk);
                    double ps = 0.0, sl;
                    int pw = 0, wl;
                    for (int p = c0; p < c1; ++p) {
                        const unsigned w = (unsigned)keys[p];
                        ps = ps + (double)word_weight(w) * tgt[word_row(w)];
                        pw += word_weight(w);
                    }
                    block_scan_excl_d(ps, pw, sl, wl);
                    double bv = -INFINITY;
                    int bp = -1;
                    if (c0 < c1) {
                        float prev = c0 > 0 ? value_of((unsigned)(keys[c0 - 1] >> 32)) : 0.0f;
                        for (int p = c0; p < c1; ++p) {
                            const unsigned long long kw = keys[p];
                            const float v = value_of((unsigned)(kw >> 32));
                            if (p > 0 && !(v <= prev + kFeatureThreshold)) {
                                const double dl = (double)wl, dr = (double)(w_node - wl), sr = sum_tot - sl;
                                double proxy;
                                if constexpr (kFried) {             // FriedmanMSE.proxy_impurity_improvement
                                    const double diff = dr * sl - dl * sr;
                                    proxy = diff * diff / (dl * dr);
                                } else {
                                    proxy = sl * sl / dl + sr * sr / dr;
                                }
                                if (proxy > bv) {
                                    bv = proxy;
                                    bp = p;
                                }
                            }
                            const unsigned w = (unsigned)kw;
                            sl = sl + (double)word_weight(w) * tgt[word_row(w)];
                            wl += word_weight(w);
                            prev = v;
                        }
                    }
                    best_of_columns(bv, bp, red_v, red_p, keys, f, best_proxy, best_f, best_thr);
                    __syncthreads();                                // (the sort words and the control block are rewritten next)
                } else if constexpr (SPLITTER == kBest) {
                    // class counts left of every candidate: per column of consecutive sorted rows, then a prefix over the columns
                    const int cols = m.hist_cols, chunk = (n_node + cols - 1) / cols;
                    const int c0 = min(n_node, tid * chunk), c1 = tid < cols ? min(n_node, c0 + chunk) : c0;
                    if (tid < cols) {
                        for (int c = 0; c < K; ++c) hist[c * pitch + tid] = 0;
                        for (int p = c0; p < c1; ++p) {
                            const unsigned w = (unsigned)keys[p];
                            hist[word_class(w) * pitch + tid] += word_weight(w);
                        }
                    }
                    __syncthreads();
                    {
                        const int lane = tid % kWave, per = cols / kWave;       // 4 or 2 columns per lane
                        for (int c = tid / kWave; c < K; c += kThreads / kWave) {
                            int *h = hist + c * pitch + lane * per;
                            int a0 = h[0], a1 = h[1], a2 = per > 2 ? h[2] : 0, a3 = per > 2 ? h[3] : 0;
                            const int s = a0 + a1 + a2 + a3;
                            int inc = s;
#pragma unroll
                            for (int o = 1; o < kWave; o <<= 1) {
                                const int u = __shfl_up(inc, o, kWave);
                                if (lane >= o) inc += u;
                            }
                            const int e0 = inc - s;
                            h[0] = e0;
                            h[1] = e0 + a0;
                            if (per > 2) {
                                h[2] = e0 + a0 + a1;
                                h[3] = e0 + a0 + a1 + a2;
                            }
                        }
                    }
                    __syncthreads();
                    double bv = -INFINITY;
                    int bp = -1;
                    if (tid < cols && c0 < c1) {
                        int wl = 0;
                        for (int c = 0; c < K; ++c) wl += hist[c * pitch + tid];
                        float prev = c0 > 0 ? value_of((unsigned)(keys[c0 - 1] >> 32)) : 0.0f;
                        for (int p = c0; p < c1; ++p) {
                            const unsigned long long kw = keys[p];
                            const float v = value_of((unsigned)(kw >> 32));
                            if (p > 0 && !(v <= prev + kFeatureThreshold)) {
                                const double dl = (double)wl, dr = (double)(w_node - wl);
                                double sql = 0.0, sqr = 0.0;
                                for (int c = 0; c < K; ++c) {
                                    const int l = hist[c * pitch + tid];
                                    const double cl = (double)l, cr = (double)(tot[c] - l);
                                    sql = sql + cl * cl;
                                    sqr = sqr + cr * cr;
                                }
                                const double gl = 1.0 - sql / (dl * dl), gr = 1.0 - sqr / (dr * dr);
                                const double proxy = -dr * gr - dl * gl;
                                if (proxy > bv) {
                                    bv = proxy;
                                    bp = p;
                                }
                            }
                            const unsigned w = (unsigned)kw;
                            hist[word_class(w) * pitch + tid] += word_weight(w);
                            wl += word_weight(w);
                            prev = v;
                        }
                    }
                    best_of_columns(bv, bp, red_v, red_p, keys, f, best_proxy, best_f, best_thr);
                    __syncthreads();                                // (the sort words and the control block are rewritten next)
                } else {
                    __syncthreads();
                    const double thr = ctl.thr;
                    int cnt = 0;
                    for (int i = start + tid; i < end; i += kThreads) {
                        const unsigned w = rows[i];
                        if ((double)xf[word_row(w)] <= thr) {
                            ++cnt;
                            atomicAdd(&left[word_class(w)], word_weight(w));
                        }
                    }
                    if (cnt) atomicAdd(&ctl.n_left, cnt);
                    __syncthreads();
                    if (tid == 0) {
                        const int nl = ctl.n_left;
                        if (nl >= 1 && n_node - nl >= 1) {          // min_samples_leaf = 1
                            int wl = 0;
                            for (int c = 0; c < K; ++c) wl += left[c];
                            const double dl = (double)wl, dr = (double)(w_node - wl);
                            double sql = 0.0, sqr = 0.0;
                            for (int c = 0; c < K; ++c) {
                                const double cl = (double)left[c], cr = (double)(tot[c] - left[c]);
                                sql = sql + cl * cl;
                                sqr = sqr + cr * cr;
                            }
                            const double gl = 1.0 - sql / (dl * dl), gr = 1.0 - sqr / (dr * dr);
                            const double proxy = -dr * gr - dl * gl;
                            if (proxy > best_proxy) {
                                best_proxy = proxy;
                                best_f = f;
                                best_thr = thr;
                            }
                        }
                    }
                    __syncthreads();                                // (left [] and the control block are rewritten next)
                }
            }
            // the known constants back in their order, the found ones behind them
            n_found = ctl.n_found;
            for (int i = tid; i < n_known; i += kThreads) feat[i] = cons[i];
            for (int i = tid; i < n_found; i += kThreads) cons[n_known + i] = feat[n_known + i];
            best_f = ctl.best_f;
            leaf = best_f < 0;
            if (!leaf) {                                            // partition_samples_final, the children's statistics
                const double thr = ctl.best_thr;
                const float *xf = xj + (long long)best_f * n;
                unsigned *tmp = reinterpret_cast<unsigned *>(keys);
                if (CRIT == kGini && tid < K) left[tid] = 0;
                const int chunk = (n_node + kThreads - 1) / kThreads, c0 = min(n_node, tid * chunk), c1 = min(n_node, c0 + chunk);
                double sum_l = 0.0, sq_l = 0.0, wn_l = 0.0;         // (MSE) the left child's sums, chunk-serial
                int cnt = 0;
                for (int i = c0; i < c1; ++i) cnt += (double)xf[word_row(rows[start + i])] <= thr;
                int lpos = block_scan_excl(cnt, s_w, n_left);
                int rpos = n_left + (c0 - lpos);
                for (int i = c0; i < c1; ++i) {
                    const unsigned w = rows[start + i];
                    if ((double)xf[word_row(w)] <= thr) {
                        tmp[lpos++] = w;
                        if constexpr (CRIT == kGini) {
                            atomicAdd(&left[word_class(w)], word_weight(w));
                        } else {
                            const double y = tgt[word_row(w)], wy = (double)word_weight(w) * y;
                            sum_l = sum_l + wy;
                            sq_l = sq_l + wy * y;
                            wn_l = wn_l + (double)word_weight(w);
                        }
                    } else {
                        tmp[rpos++] = w;
                    }
                }
                __syncthreads();
                for (int i = tid; i < n_node; i += kThreads) rows[start + i] = tmp[i];
                if constexpr (kReg) block_sum3(sum_l, sq_l, wn_l);
                if (tid == 0) {
                    if (n_left < 1 || n_left >= n_node) {
                        leaf = 1;                                   // (cannot happen with finite values)
                    } else if constexpr (kReg) {                   // MSE.children_impurity
                        const double dl = wn_l, dn = (double)w_node, dr = dn - dl, sum_r = sum_tot - sum_l;
                        imp_l = sq_l / dl - (sum_l / dl) * (sum_l / dl);
                        imp_r = (sq_tot - sq_l) / dr - (sum_r / dr) * (sum_r / dr);
                        double improvement;
                        if constexpr (kFried) {                     // FriedmanMSE.impurity_improvement (one output)
                            const double diff = dr * sum_l - dl * sum_r;
                            improvement = diff * diff / (dl * dr * dn);
                        } else {
                            improvement = (dn / w_total) * (impurity - (dr / dn * imp_r) - (dl / dn * imp_l));
                        }
                        leaf = improvement + DBL_EPSILON < 0.0;
                    } else {
                        int wl = 0;
                        for (int c = 0; c < K; ++c) wl += left[c];
                        const double dl = (double)wl, dr = (double)(w_node - wl), dn = (double)w_node;
                        double sql = 0.0, sqr = 0.0;
                        for (int c = 0; c < K; ++c) {
                            const double cl = (double)left[c], cr = (double)(tot[c] - left[c]);
                            sql = sql + cl * cl;
                            sqr = sqr + cr * cr;
                        }
                        imp_l = 1.0 - sql / (dl * dl);
                        imp_r = 1.0 - sqr / (dr * dr);
                        const double improvement = (dn / w_total) * (impurity - (dr / dn * imp_r) - (dl / dn * imp_l));
                        leaf = improvement + DBL_EPSILON < 0.0;
                    }
                }
            }
            __syncthreads();
        }
        // the node's record; the next node
        if (tid == 0) {
            const long long g = task.node_off + node;
            const double thr = ctl.best_thr;
            if (node + 3 + sp > task.cap) leaf = 1;                 // (two children and every pending node fit: always, by the row counts)
            const int missing = !leaf && n_left > n_node - n_left;
            if (ctl.parent >= 0 && !ctl.is_left) m.nodes[task.node_off + ctl.parent].next = task.node_rel + node;
            forest::Node nd;
            nd.threshold = leaf ? 0.0 : thr;
            nd.meta = leaf ? forest::kLeaf : (best_f | (missing ? forest::kMissingLeft : 0));
            nd.next = leaf ? task.node_rel + node : -1;
            m.nodes[g] = nd;
            if (m.children_left) {
                if (ctl.parent >= 0) (ctl.is_left ? m.children_left : m.children_right)[task.node_off + ctl.parent] = node;
                m.children_left[g] = -1;
                m.children_right[g] = -1;
                m.feature[g] = leaf ? -2 : best_f;
                m.threshold[g] = leaf ? -2.0 : thr;
                m.impurity[g] = impurity;
                m.n_node_samples[g] = n_node;
                m.weighted_n_node_samples[g] = (double)w_node;
                m.missing_go_to_left[g] = (unsigned char)missing;
            }
            if (!leaf) {
                stack[sp].start = start + n_left;
                stack[sp].end = end;
                stack[sp].parent = kFried ? node | ((depth + 1) << 16) : node;     // (a node id is below 2^15)
                stack[sp].n_known = n_total;
                stack[sp].impurity = imp_r;
                ++sp;
                ctl.end = start + n_left;
                ctl.parent = node;
                ctl.is_left = 1;
                ctl.n_known = n_total;
                impurity = imp_l;
                ++depth;
            } else if (sp > 0) {
                --sp;
                ctl.start = stack[sp].start;
                ctl.end = stack[sp].end;
                ctl.parent = kFried ? stack[sp].parent & 0xffff : stack[sp].parent;
                depth = kFried ? stack[sp].parent >> 16 : 0;
                ctl.is_left = 0;
                ctl.n_known = stack[sp].n_known;
                impurity = stack[sp].impurity;
            } else {
                ctl.done = 1;
                m.node_count[blockIdx.x] = node + 1;
            }
            ctl.node = node + 1;
            if constexpr (kFried) ctl.closed = leaf;                // (a field of its own: ctl.leaf is read by the other waves without a barrier after this)
        }
        __syncthreads();
        if constexpr (kFried) {
            // _update_terminal_regions of the closed leaf: one Newton step over its rows, then the raw predictions of those rows
            if (m.raw != nullptr && ctl.closed) {                   // (written before the barrier above; next written after the leaf step's own barriers)
                const BoostTask bt = m.boost[blockIdx.x];
                const int chunk = (n_node + kThreads - 1) / kThreads, c0 = min(n_node, tid * chunk), c1 = min(n_node, c0 + chunk);
                double den = 0.0, z0 = 0.0, z1 = 0.0;
                for (int i = c0; i < c1; ++i) {
                    const int r = word_row(rows[start + i]);
                    const double p = (lab[r] == bt.cls ? 1.0 : 0.0) - tgt[r];
                    den = den + p * (1.0 - p);
                }
                block_sum3(den, z0, z1);
                double num = sum_tot / (double)n_node;
                num = num * bt.factor;                              // (K - 1) / K; 1.0 for the two-class loss
                den = den / (double)n_node;
                const double value = fabs(den) < 1e-150 ? 0.0 : num / den;
                const double step = m.learning_rate * value;
                if (tid == 0) m.value[task.val_off + node] = value;
                for (int i = start + tid; i < end; i += kThreads) {
                    const long long at = bt.off + word_row(rows[i]);
                    m.raw[at] = m.raw[at] + step;
                }
            }
        }
        if (ctl.done) break;
    }
}
#pragma clang fp contract(fast)

}  // namespace treefit
}  // namespace paa
