// Limits, device records and launch entry points of the model families (svc, svr with svrfit, knn, smo, forest, hmm, diar, lda).  Every family
// is its own translation unit (family_<name>.hip: its kernels and the host code that picks an instance are there and
// nowhere else); the host side of the library (the lib_*.hpp units of paa_lib.hip) sees only what is here.  Every launch::
// function queues its kernels on `stream` and returns 0, or -1 when a launch failed (hipGetLastError has the reason).
// No device code.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

namespace paa {
namespace svc {
constexpr int kMaxClasses = 16;
constexpr int kMaxDims = 256;
// one uploaded model (libsvm's svm_model as scikit-learn holds it): device pointers
struct SvcDev {
    const double *sv;         // [n_sv][n_dims] support vectors, grouped by class
    const double *coef;       // [k - 1][n_sv] sv_coef (scikit-learn's _dual_coef_)
    const int *class_end;     // [k] end of class c's range of support vectors (cumulative n_support)
    const double *rho;        // [k (k - 1) / 2] (= -_intercept_)
    const double *prob_a, *prob_b;
    int n_sv, n_dims, k, rbf;
    double gamma;
};
}  // namespace svc
namespace svr {
constexpr int kMaxModels = 4096;
constexpr int kMaxDims = 256;
// one uploaded bank of epsilon-SVR models that share n_dims (libsvm's svm_model as scikit-learn holds it): device pointers
struct SvrDev {
    const double *sv;         // [total_sv][n_dims] support vectors, model after model
    const double *coef;       // [total_sv] sv_coef (scikit-learn's _dual_coef_[0])
    const long long *sv_off;  // [n_models + 1] model m owns support vectors sv_off[m] .. sv_off[m + 1] - 1 (none: legal)
    const double *rho;        // [n_models] (= -_intercept_)
    const double *gamma;      // [n_models]
    const int *rbf;           // [n_models] 1: RBF, 0: linear
    const int *same_prev;     // [n_models] 1: mean / std of model m equal those of model m - 1 bit for bit
    const double *mean, *scale;   // [n_models][n_dims] every model's own standardisation
    int n_models, n_dims;
};
}  // namespace svr
namespace knn {
constexpr int kMaxK = 32;
constexpr int kMaxClasses = 64;
constexpr int kMaxDims = 256;
constexpr int kQueriesPerBlock = 16;      // kernels_knn.hpp: one query per group of lanes
// one uploaded kNN model (audioTrainTest.Knn): device pointers
struct KnnDev {
    const double *train;      // [n_train][n_dims] training vectors
    const int *labels;        // [n_train] class index of every row (a value outside 0..n_classes-1 votes for no class)
    int n_train, n_dims, n_classes, k;
};
// a sweep of kNN jobs over ONE sample matrix (audioTrainTest.evaluate_classifier's splits): job j trains on the rows
// train_idx[train_off[j] .. train_off[j + 1] - 1] of X and classifies the rows test_idx[test_off[j] .. test_off[j + 1] - 1], both
// after its own (x - mean_j) / scale_j, with its own k_j and n_classes_j.  Device pointers
struct SplitBlock {
    int job, first;           // a workgroup's job and the position in that job's test list of its first query
};
struct KnnSplitDev {
    const double *X;          // [n_samples][n_dims] every sample, row-major
    const int *labels;        // [n_samples] class index of every sample (a value outside 0..n_classes_j-1 votes for no class)
    const long long *train_off, *test_off;    // [n_jobs + 1], from 0
    const int *train_idx, *test_idx;          // sample indices, job after job
    const double *mean, *scale;               // [n_jobs][n_dims]
    const int *k, *n_classes;                 // [n_jobs]
    const SplitBlock *blocks;                 // [n_blocks] host-built grid
    int n_dims, max_classes;
};
constexpr int kSplitKs[] = {1, 2, 4, 8, 16, 32};      // the instances of knn_split_kernel: a sweep runs at the smallest >= its largest k
}  // namespace knn
namespace smo {
constexpr int kThreads = 256;             // kernels_smo.hpp: one workgroup per task, 32 groups of 8 lanes
constexpr int kGroups = 32;
constexpr int kMaxRows = 8192;            // rows of a task: its kernel row K_it stays in LDS (64 KB)
constexpr int kMaxDims = 256;
constexpr int kMaxClasses = 64;           // classes present in one job of a sweep
constexpr int kQueriesPerBlock = 32;      // svc_pairs_kernel: one test row per group
constexpr int kDefaultItersPerLaunch = 1024;
enum Status { kFresh = 0, kRunning = 1, kConverged = 2, kNotConverged = 3 };
// one binary C-SVC dual problem over rows of the resident sample matrix
struct SmoTask {
    long long off;            // its rows are idx[off .. off + n - 1], with sign[off ..]
    int n, stat;              // stat: the row of mean / scale it standardises with
    double C, gamma;
};
// a batch of tasks and their state: device pointers
struct SmoDev {
    const double *X;          // [n_samples][n_dims]
    const int *idx;           // sample index of every row of every task
    const signed char *sign;  // +1: the first class of the pair, -1: the second
    const SmoTask *tasks;
    const double *mean, *scale;   // [..][n_dims]
    double *alpha, *G, *QD;   // state per row: alpha, the gradient, K_tt
    double *alpha_y;          // out per row, written at a task's stop: alpha_t y_t
    int *iter, *status;       // state per task (status: Status)
    double *rho, *gap;        // out per task
    int *n_sv;                // out per task: rows with alpha != 0
    int n_dims, rbf, max_iter;
    double eps;
};
// the resident kernel matrices of a chunk of groups (kernels_smocache.hpp).  A group is a set of tasks with one mean / scale / gamma; its
// matrix K [N][N] runs over the group's distinct rows.  Per task: k_off, where its group's matrix begins in K (in doubles, 64-bit: a
// chunk may pass 4 GiB), and group_n, that matrix's N; per row of every task (at the task's off): pos, its row of the matrix
struct SmoCacheDev {
    const double *K;
    const long long *k_off;   // [n_tasks]; read for the tasks of the current chunk only
    const int *group_n;       // [n_tasks]
    const int *pos;
};
// the fitted tasks of a split sweep and its test lists (job j owns the tasks job_task[j] .. job_task[j + 1] - 1, the pairs
// (a, b), a < b, of its job_k[j] present classes in row-major order): device pointers
struct SvcFitDev {
    const double *X;
    const long long *test_off;
    const int *test_idx;
    const knn::SplitBlock *blocks;
    const int *job_task, *job_k;
    const int *job_stat;          // [n_jobs] the row of mean / scale a job standardises with (null: its own index)
    const double *mean, *scale;   // [..][n_dims]
    const SmoTask *tasks;
    const int *idx;
    const double *alpha_y, *rho;
    int n_dims, rbf, max_pairs;
};
}  // namespace smo
namespace platt {
constexpr int kThreads = 256;             // kernels_platt.hpp: one workgroup per problem (the held-out values of one class pair)
constexpr int kMaxRows = smo::kMaxRows;   // values of a problem: they stay in LDS with their signs (72 KB)
constexpr int kMaxIter = 100;             // sigmoid_train's constants (svm.cpp)
constexpr int kMaxHalvings = 34;          // step 1, 1/2, ... 2^-33: the steps >= kMinStep
constexpr double kMinStep = 1e-10, kSigma = 1e-12, kEps = 1e-5;
enum Stop { kConverged = 0, kLineSearchFailed = 1, kMaxIterations = 2 };
// a batch of sigmoid fits: device pointers.  Problem p owns dec / sign [off[p] .. off[p + 1] - 1]
struct PlattDev {
    const double *dec;
    const signed char *sign;  // +1: the pair's first class, -1: the second
    const long long *off;     // [n_problems + 1]
    double *A, *B;            // out per problem
    int *iter, *stop;         // out per problem: Newton iterations; Stop
};
}  // namespace platt
namespace onset {
constexpr int kThreads = 256;             // kernels_onset.hpp: one workgroup per clip (one thread per frame in onset_proba_kernel)
constexpr int kMaxDims = 256;             // feature rows of a short-term matrix (a thread per row forms the scaler)
// a clip of a silence-removal batch: its short-term matrix [n_dims][T] at feats + feat_off, its frames at frame_off in every
// per-frame array; after stage 1 the host fills the counts and row_off, the clip's first row in the training matrix
struct ClipRec {
    long long feat_off, frame_off, row_off;
    int T, n_quiet, n_loud, width;        // width: the smoothing box in frames
    double weight;                        // of the highest tenth in the threshold
};
// a batch: device pointers.  Per frame: quiet, loud, raw, prob, active; per clip: limits [2], counts [2], mean / scale / w
// [n_dims], rho, intercept, A, B, thr; per training row: src (its frame), X [n_dims], alpha_y
struct OnsetDev {
    const double *feats;
    const ClipRec *clips;
    double *limits;
    int *counts;
    unsigned char *quiet, *loud, *active;
    int *src;
    double *X, *mean, *scale;
    const double *alpha_y, *rho;
    double *w, *intercept;
    const double *A, *B;
    double *raw, *prob, *thr;
    int n_dims;
};
}  // namespace onset
namespace svrfit {
// a batch of epsilon-SVR dual problems and their state (kernels_svrfit.hpp): device pointers.  A task is an smo::SmoTask (its n rows
// are idx[off ..]); its 2 n dual variables -- variable v stands for row v mod n, with the sign +1 for v < n and -1 for v >= n --
// have their alpha and G at 2 off .. 2 off + 2 n - 1; K_tt, beta and the training predictions are per row, at off
struct SvrDev {
    const double *X;          // [n_samples][n_dims]
    const double *y;          // [n_samples]: the targets
    const int *idx;           // sample index of every row of every task
    const smo::SmoTask *tasks;
    const double *epsilon;    // [n_tasks]: the width of the tube
    const double *mean, *scale;   // [..][n_dims]
    double *alpha, *G;        // state per variable
    double *QD;               // state per row: K_tt
    double *beta, *train_pred;    // out per row, written at a task's stop: alpha_t - alpha_{t+n}; sum_s beta_s K_ts - rho
    int *iter, *status;       // state per task (status: smo::Status)
    double *rho, *gap;        // out per task
    int *n_sv;                // out per task: rows with beta != 0
    int n_dims, rbf, max_iter;
    double eps;
};
// the resident kernel matrices of a chunk of tasks (kernels_svrcache.hpp): Z [n][pitch], a task's standardised rows (pitch = 8 ceil(n_dims
// / 8), zero beyond n_dims), at z_off[task]; K [n][n], full, at k_off[task].  Offsets count doubles and are 64-bit: a chunk may pass 4 GiB
constexpr int kGramTile = 32;             // svr_gram_kernel: rows of a tile, one per 8-lane group of the workgroup
constexpr int kPitchLanes = 8;            // kv::kGroupLanes: a row of Z is padded to a multiple of it
constexpr int kGramMaxRows = 65535 * kGramTile;   // rows of a matrix: svr_standardise_kernel's grid has a block row per tile of rows
struct SvrCacheDev {
    double *Z, *K;
    const long long *z_off, *k_off;       // [n_tasks]; read for the tasks of the current chunk only
};
// a workgroup of svr_gram_kernel: the tile pair (a, b), a <= b, of a task
struct GramTile {
    int task, a, b;
};
}  // namespace svrfit
namespace forest {
constexpr int kMaxClasses = 64;
constexpr int kMaxDims = 256;
constexpr int kWin = 64;                  // kernels_forest.hpp: windows per traversal workgroup, one per lane
constexpr int kChunk = 32768;             // windows per traversal / reduction pass (bounds the leaf-slot scratch)
// a packed tree node (preorder: the left child of node i is node i + 1): 16 bytes, one load per visited node
constexpr int kFeatureMask = 0xffff, kMissingLeft = 1 << 16, kLeaf = 1 << 17;
struct Node {
    double threshold;         // go left when (double)x32[feature] <= threshold
    int meta;                 // feature | kMissingLeft (NaN goes left) | kLeaf
    int next;                 // internal: the right child's node index; leaf: its leaf slot (row of leaf_values)
};
// one uploaded tree ensemble (scikit-learn's RandomForest / ExtraTrees / GradientBoosting classifiers): device pointers
struct ForestDev {
    const Node *nodes;        // every tree's nodes, tree after tree, each in preorder
    const int *roots;         // [n_trees] node index of every root
    const double *leaf_values;    // [n_leaves][n_outputs] averaged forest: class fractions; boosted: [n_leaves] values
    const double *init;       // [n_outputs] boosted: the constant initial raw score
    int n_trees, n_dims, n_classes, n_outputs, boosted;
    double learning_rate;
};
}  // namespace forest
namespace treefit {
constexpr int kThreads = 256;             // kernels_treefit.hpp: one workgroup per tree
constexpr int kMaxRows = 8192;            // rows of a job's training list: a row's place, class and weight share one 32-bit word
constexpr int kMaxClasses = forest::kMaxClasses;
constexpr int kMaxDims = forest::kMaxDims;
constexpr int kMaxWeight = 8191;          // a row's integer weight (0: out of the bag)
constexpr long long kChunkBytes = 1LL << 30;      // device scratch of one chunk of a sweep's trees (a job is never cut)
enum Splitter { kBest = 0, kRandom = 1 };
enum Criterion { kGini = 0, kMse = 1, kFriedman = 2 };    // classification; regression (squared error, one output, best splitter);
                                                          // a boosting stage's tree (Friedman's improvement over the squared-error sums, a depth limit)
// a job: the rows idx[off .. off + n - 1] of the sample matrix, their class indices label[off ..] in 0 .. k - 1, standardised
// with row `stat` of mean / scale; its float32 copy x32[x_off ..] is feature-major [n_dims][n]
struct TreeJob {
    long long off, x_off;
    int n, k, stat, pad;
};
// a tree: its job, the rand_r seed, the weights weight[w_off .. w_off + n - 1] of the job's rows (w_off < 0: every row 1) and
// its place in the outputs: nodes at node_off (room for cap = 2 in-bag rows - 1), values at val_off; the packed nodes count
// from node_rel (the tree's first node among the nodes of its job's trees)
struct TreeTask {
    long long w_off, node_off, val_off;
    int job, cap, node_rel;
    unsigned seed;
};
// a pending right child of the depth-first build
struct StackRec {
    int start, end, parent, n_known;
    double impurity;
};
// a boosting stage's tree (kFriedman, the sweep): its residuals are target[off .. off + n - 1] and the raw predictions it steps
// raw[off ..], by the job's rows; cls: the class whose tree it is (the two-class loss: 1); factor: (K - 1) / K, 1.0 for two classes
struct BoostTask {
    long long off;
    double factor;
    int cls, pad;
};
// a batch of trees: device pointers.  The scikit-learn arrays (children_left .. missing) may be null: the sweep keeps the packed
// nodes and the values only
struct TreeDev {
    const double *X;          // [n_samples][n_dims]
    const int *idx, *label;   // per job row (label: kGini)
    const double *target;     // per job row (kMse; such a job has k = 1)
    const TreeJob *jobs;
    const TreeTask *tasks;
    const int *weight;
    const double *mean, *scale;   // [..][n_dims]
    float *x32;               // prep: every job's standardised float32 rows
    int *flags;               // prep, per job: 1: a value is infinite in float32, 2: a value is NaN
    StackRec *stack;          // [total cap]
    forest::Node *nodes;      // out [total cap]: forest_traverse_kernel's layout
    double *value;            // out: per node the class fractions, [cap][k of the job] per tree; kMse: the weighted mean, [cap]
    int *node_count;          // out per task
    int *children_left, *children_right, *feature, *n_node_samples;
    double *threshold, *impurity, *weighted_n_node_samples;
    unsigned char *missing_go_to_left;
    int n_dims, max_features;
    int lds_keys, lds_rows, hist_cols, lds_feat;      // LDS geometry of the launch: 8-byte sort words, row words, columns of the class
                                                      // histogram, byte offset of the feature arrays
    // kFriedman: a node at max_depth is a leaf (the root has depth 0).  With boost / raw (the sweep; null: the builder alone) task t
    // reads its targets through boost[t], and a closed leaf takes its Newton value and adds learning_rate * value to its rows of raw
    int max_depth, pad;
    const BoostTask *boost;
    double *raw;
    double learning_rate;
};
}  // namespace treefit
namespace boost {
constexpr int kThreads = 256;             // kernels_boost.hpp: one workgroup per job
// a job of a boosting sweep: its rows' class indices label[off .. off + n - 1] in 0 .. k - 1, its raw predictions and residuals
// [k_out][n] at r_off (k_out = 1 for two classes, else k), its initial raw score init[init_off ..], its losses loss[loss_off + stage]
struct BoostJob {
    long long off, r_off, loss_off, init_off;
    int n, k, n_stages, pad;
};
struct BoostDev {
    const BoostJob *jobs;
    const int *label;
    const double *init;
    double *raw, *resid, *loss;
};
}  // namespace boost
namespace hmm {
constexpr int kMaxStates = 32;
constexpr int kMaxDims = 256;
constexpr int kBlockRows = 256;           // rows per segment of a long sequence (kernels_hmm.hpp); shorter sequences are one segment
// one uploaded Gaussian HMM (diagonal): device pointers; kp = n_states rounded up to a power of two (>= 2), padded
// states have log-probability -inf
struct HmmDev {
    const double *mu, *inv;   // [n_dims][kp] means and 1 / covars_ (the reference's covars_ hold standard deviations)
    const double *cst;        // [kp] n_dims log(2 pi) + sum_d log covars_[k][d]
    const double *logpi;      // [kp] log startprob
    const double *logA;       // [kp][kp] log transmat
    int n_states, n_dims, kp;
};
// rows r0 .. r1 - 1 of the stacked sequences; first / last: the segment begins / ends its sequence
struct Segment {
    long long r0, r1;
    int first, last;
};
}  // namespace hmm
namespace diar {
// k-means of one k of a sweep (kernels_diar.hpp): written by finish_kernel, polled by the host after every iteration
struct KmState {
    int done, strict, n_iter, n_empty;
    double shift;
};
constexpr int kMaxPoints = 8;                         // candidate windows per sqdist_points_kernel launch
constexpr int kIntsPerK = hmm::kMaxStates + 1;      // cluster sizes and the number of changed labels of one assignment
// The records of a batch of clips (kernels_diarbatch.hpp).  Every clip is the column range [col, col + n) of one matrix
// [n_dims][ld]; its kept feature rows are rows[rows_off .. rows_off + D - 1]; its (clip, k) jobs are consecutive.  Offsets are
// in elements of the array they index.
constexpr int kBatchPairTile = 128;                   // windows per side of a pair tile, as kPairTile of kernels_diar.hpp
constexpr int kBatchTrials = 5;                       // 2 + int(ln 32) k-means++ candidates per step at most
struct BatchClip {
    long long col, n, lab_off;          // lab_off: the labels of the clip's first job ([nk][n] from there)
    int D, rows_off, first_job, nk, bin_tab, pad;
};
struct BatchJob {
    long long col, n, lab_off, tmp_off, u_off, cen_off, first;
    double tol;
    int D, rows_off, k, seeded, trials, pad;
};
struct BatchSlot {                      // the feature-row distances over the windows labelled `cluster` (lab_off < 0: all)
    long long col, n, lab_off, dist_off, sum_off;
    int D, rows_off, cluster, pad;      // rows_off < 0: rows 0 .. D - 1
};
struct BatchTile {
    long long part_off;
    int clip, bi, bj, pad;
};
struct BatchRed {
    long long in_off, rows, out_off;
    int nbins, pad;
};
}  // namespace diar

// f(std::integral_constant<int, v>) for Lo <= v <= Hi, one instance per value; -1 outside the range
template <int Lo, int Hi, typename F>
int dispatch_int(int v, F &&f) {
    if (v == Lo) return f(std::integral_constant<int, Lo>{});
    if constexpr (Lo < Hi) return dispatch_int<Lo + 1, Hi>(v, std::forward<F>(f));
    return -1;
}

namespace launch {

// for a launch unit: lets `kernel` take `lds` bytes of dynamic LDS (above 32 KB a kernel has to be told); 0, or -1 when refused
inline int raise_lds(const void *kernel, size_t lds) {
    if (lds <= 32 * 1024) return 0;
    return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess ? 0 : -1;
}

// kernels_svc.hpp: multi-class probabilistic SVC over the columns of feats [n_dims][ld] (two kernels: the per-class sums go to
// `sums`, n_vec * k * (k - 1) doubles; then labels [n_vec] and probabilities [n_vec][k])
int svc(const svc::SvcDev &m, const double *d_feats, long long ld, long long n_vec, const double *d_mean, const double *d_scale,
        double *d_sums, int *d_label, double *d_proba, hipStream_t stream);
// kernels_svr.hpp: a bank of epsilon-SVR models over the columns of feats [n_dims][ld] (one kernel): out [n_models][ld_out], every
// model's prediction of every column after that model's own (x - mean) / std
int svr(const svr::SvrDev &m, const double *d_feats, long long ld, long long n_vec, double *d_out, long long ld_out,
        hipStream_t stream);
// ... and its geometry, for tests that aim at its edges: windows per workgroup, models per workgroup, support vectors per tile, lanes per group
void svr_geometry(int out4[4]);
// kernels_knn.hpp: k-nearest-neighbour classification of the columns of feats [n_dims][ld] (one kernel: labels [n_vec],
// P [n_vec][n_classes] and, when d_neighbors is not null, the k neighbour indices [n_vec][k] in ascending (d^2, index))
int knn(const knn::KnnDev &m, const double *d_feats, long long ld, long long n_vec, const double *d_mean, const double *d_scale,
        int *d_label, double *d_proba, int *d_neighbors, hipStream_t stream);
// kernels_knn.hpp: a sweep of kNN jobs over one sample matrix (one kernel, n_blocks workgroups of the host-built table
// m.blocks; k_max: the largest k of the sweep): labels [Q], P [Q][max_classes] when d_proba is not null (zeros at and beyond a
// job's n_classes), the neighbours' train-list positions [Q][k_launch] when d_neighbors is not null (-1 past a job's k or
// train list), Q test vectors in job order then test-list order, in ascending (d^2, train-list position)
int knn_split(const knn::KnnSplitDev &m, long long n_blocks, int k_max, int *d_label, double *d_proba, int *d_neighbors,
              hipStream_t stream);
// ... the instance a sweep with that largest k runs at (0: none), and the geometry for tests that aim at its edges: queries per
// workgroup, training rows per LDS tile, rows per step (= lanes per query), the number of K instances and the instances
int knn_split_k_launch(int k_max);
void knn_split_geometry(int out10[10]);
// kernels_smo.hpp: at most `budget` SMO iterations of each of the n_live tasks d_live [n_live] of the batch m (one workgroup
// each; n_max: the longest of them, which sizes the LDS); -2 when n_max or n_dims exceeds the limits
int smo_step(const smo::SmoDev &m, const int *d_live, int n_live, int n_max, int budget, hipStream_t stream);
// kernels_smocache.hpp: smo_step over the resident matrices c (no LDS row: n_max is not bounded)
int smo_cached_step(const smo::SmoDev &m, const smo::SmoCacheDev &c, const int *d_live, int n_live, int budget, hipStream_t stream);
// ... and the one-against-one vote over fitted tasks: labels [Q] (position among the job's classes) and, when d_dec is not null,
// decision values [Q][max_pairs]
int svc_pairs(const smo::SvcFitDev &f, long long n_blocks, int *d_label, double *d_dec, hipStream_t stream);
// ... the geometry for tests that aim at its edges: threads per workgroup, groups, the row limit, test rows per scoring
// workgroup, the default iterations per launch, the dims limit
void smo_geometry(int out6[6]);
// kernels_platt.hpp: libsvm's sigmoid_train for each of the n_problems problems of p (one workgroup each; l_max: the longest
// of them, which sizes the LDS); -2 when l_max exceeds platt::kMaxRows
int platt_sigmoid(const platt::PlattDev &p, int n_problems, int l_max, hipStream_t stream);
// kernels_onset.hpp (silence removal of a batch of clips): the energy limits, flags and counts of every clip; ...
int onset_select(const onset::OnsetDev &m, int n_clips, hipStream_t stream);
// ... the training rows, their matrix and its scaler (the clip records carry the counts and row offsets)
int onset_gather(const onset::OnsetDev &m, int n_clips, hipStream_t stream);
// ... the fits (alpha_y, rho) folded into w and intercept
int onset_weights(const onset::OnsetDev &m, int n_clips, hipStream_t stream);
// ... the onset probability raw of every one of the batch's n_frames frames
int onset_proba(const onset::OnsetDev &m, int n_clips, long long n_frames, hipStream_t stream);
// ... smoothing, threshold and activity flags
int onset_threshold(const onset::OnsetDev &m, int n_clips, hipStream_t stream);
// kernels_svrfit.hpp: smo_step for a batch of epsilon-SVR tasks (the limits are the SMO solver's)
int svr_smo_step(const svrfit::SvrDev &m, const int *d_live, int n_live, int n_max, int budget, hipStream_t stream);
// kernels_svrcache.hpp: Z then K of the n_chunk tasks listed in d_chunk (n_max: the longest of them, at most svrfit::kGramMaxRows; d_tiles:
// every tile pair of every one of them), and svr_smo_step over resident matrices.  The C-SVC solver forms its groups' matrices with
// the same call: a group's row list is a task here (lib_gramcache.hpp)
int svr_gram(const svrfit::SvrDev &m, const svrfit::SvrCacheDev &c, const int *d_chunk, int n_chunk, int n_max,
             const svrfit::GramTile *d_tiles, long long n_tiles, hipStream_t stream);
int svr_smo_cached_step(const svrfit::SvrDev &m, const svrfit::SvrCacheDev &c, const int *d_live, int n_live, int n_max, int budget,
                        hipStream_t stream);
// kernels_forest.hpp: tree-ensemble classification of the columns of feats [n_dims][ld] (per chunk of forest::kChunk windows
// two kernels: every (window, tree)'s leaf slot goes to `leaves` [n_trees][kChunk]; then labels [n_vec] (-1: a value is
// infinite in float32, -2: boosted and a value is NaN), the tree sums / raw scores raw [n_vec][n_outputs] and the
// probabilities proba [n_vec][n_classes])
int forest(const forest::ForestDev &m, const double *d_feats, long long ld, long long n_vec, const double *d_mean,
           const double *d_scale, int *d_leaves, int *d_label, double *d_raw, double *d_proba, hipStream_t stream);
// kernels_treefit.hpp: the float32 copies of n_jobs jobs (n_max: the longest of them) and their flags (zeroed here)
int tree_prep(const treefit::TreeDev &m, int n_jobs, int n_max, hipStream_t stream);
// ... one workgroup per task builds its tree (splitter: treefit::Splitter; inbag_max: the most in-bag rows of a task, k_max the
// most classes of a job; they size the LDS and are written into m); -2 when a limit is exceeded
int tree_fit(treefit::TreeDev &m, int n_tasks, int splitter, int inbag_max, int k_max, hipStream_t stream);
// ... the same for regression trees (treefit::kMse over the best splitter; m.target in place of m.label, every job's k is 1)
int tree_fit_reg(treefit::TreeDev &m, int n_tasks, int inbag_max, hipStream_t stream);
// ... the same for the trees of boosting stages (treefit::kFriedman over the best splitter, m.max_depth; tasks, boost records and
// node counts are read from m's pointers as given, so a stage launches at its first task).  configure: size the LDS for inbag_max and
// write the geometry into m; false for the later stages of a chunk, whose geometry m already holds
int tree_fit_boost(treefit::TreeDev &m, int n_tasks, int inbag_max, hipStream_t stream, bool configure = true);
// kernels_boost.hpp: for each of the first n_jobs jobs, at `stage`: the mean loss of the raw predictions (stage > 0: to loss[stage -
// 1]) and, while stage < n_stages, the negative gradients of the stage's trees (stage 0 writes the initial raw predictions first)
int boost_gradient(const boost::BoostDev &m, int n_jobs, int stage, hipStream_t stream);
// ... out [n_dims][ld] = the rows d_rows [n_rows] of X [..][n_dims], feature-major as the traversal kernel reads them
int tree_gather(const double *d_X, int n_dims, const int *d_rows, long long n_rows, double *d_out, long long ld, hipStream_t stream);
// ... threads per workgroup, the row limit, the class limit, the dims limit, the weight limit, the chunk size in MiB
void tree_fit_geometry(int out6[6]);
// kernels_hmm.hpp: frame log-likelihoods loglik [n_vec][n_states] of the columns of feats [n_dims][ld] (one kernel)
int hmm_emission(const hmm::HmmDev &m, const double *d_feats, long long ld, long long n_vec, double *d_loglik, hipStream_t stream);
// ... and Viterbi over n_seq sequences cut into n_seg segments (segment s of sequence q: seq_seg[q] <= s < seq_seg[q + 1]):
// states [rows] and logprob [n_seq].  multi: some sequence has more than one segment (two more kernels: M [n_seg][kp][kp],
// V [n_seg][kp]); Vout [n_seg][kp], psi [rows][kp] bytes, emap [n_seg][kp] bytes, seg_end [n_seg] are scratch
int hmm_decode(const hmm::HmmDev &m, const double *d_loglik, const hmm::Segment *d_segs, long long n_seg,
               const long long *d_seq_seg, long long n_seq, int multi, double *d_M, double *d_V, double *d_Vout,
               unsigned char *d_psi, unsigned char *d_emap, int *d_seg_end, int *d_states, double *d_logprob, hipStream_t stream);
// ... and the training statistics of labelled windows: counts [K + K K] (zero on entry: class counts, transition counts),
// means / stds [K][n_dims] (two kernels)
int hmm_stats(const double *d_feats, long long ld, long long n_vec, const int *d_labels, int n_states, int n_dims,
              int *d_counts, double *d_means, double *d_stds, hipStream_t stream);
// kernels_diar.hpp (speaker diarization); every matrix feature-major [n_dims][ld].  Z = StandardScaler of M, stats [3][n_dims]
int diar_standardize(const double *d_M, long long ldm, long long n, int n_dims, double *d_Z, long long ldz, double *d_stats,
                     hipStream_t stream);
// out [n_rows][ldo] = the rows `d_rows` of Z
int diar_select_rows(const double *d_Z, long long ldz, long long n, const int *d_rows, int n_rows, double *d_out, long long ldo,
                     hipStream_t stream);
// distances between feature rows over the windows labelled c of sweep entry kidx (d_labels [nk][n]; null: all windows, nk =
// kmax = 1): dist [nk][kmax][D][D] (scratch), colsum [nk][kmax][D], pmean [nk][kmax]
int diar_dim_distances(const double *d_Z, long long ld, long long n, int D, const int *d_labels, const int *d_ks, int nk, int kmax,
                       double *d_dist, double *d_colsum, double *d_pmean, hipStream_t stream);
// one Lloyd iteration of every unfinished k (ints [nk][33] is zeroed here), and the last pass (labels, d2, inertia [nk])
int diar_kmeans_step(const double *d_Zk, long long ld, long long n, int D, const int *d_ks, int nk, int kmax, double *d_centers,
                     diar::KmState *d_state, int *d_labels, double *d_d2, int *d_ints, double *d_sums, double tol, int max_iter,
                     hipStream_t stream);
int diar_kmeans_last(const double *d_Zk, long long ld, long long n, int D, const int *d_ks, int nk, int kmax, const double *d_centers,
                     const diar::KmState *d_state, int *d_labels, double *d_d2, double *d_inertia, hipStream_t stream);
int diar_sqdist_points(const double *d_Zk, long long ld, long long n, int D, const long long *d_idx, int n_pts, double *d_out,
                       hipStream_t stream);
int diar_get_points(const double *d_Zk, long long ld, int D, const long long *d_idx, int n_pts, double *d_out, hipStream_t stream);
// cluster-pair distance sums of every k of a sweep in one pass: S [binoff[nk]] (per k: [K][K]); partial and stage are scratch
// of diar_pair_tiles(n) * nbins and diar_pair_chunks(n) * nbins doubles
long long diar_pair_tiles(long long n);
long long diar_pair_chunks(long long n);
int diar_pair_sums(const double *d_Zk, long long ld, long long n, int D, const int *d_labels, const int *d_ks, int nk,
                   const int *d_binoff, int nbins, double *d_partial, double *d_stage, double *d_S, hipStream_t stream);
// kernels_diarbatch.hpp (speaker diarization of a batch of clips); the records are diar::Batch* arrays on the device
constexpr long long kDiarbPairChunk = 256;            // tiles added up by one thread of the first reduction stage, as the single call
int diarb_standardize(const double *d_M, long long ld, const diar::BatchClip *d_clips, int n_clips, int n_dims, double *d_Z,
                      double *d_stats, hipStream_t stream);
// dist is scratch (slot.dist_off); colsum at slot.sum_off, pmean [n_slots]; max_D: the widest slot
int diarb_dim_distances(const double *d_Z, long long ld, const int *d_rows, const diar::BatchSlot *d_slots, int n_slots, int max_D,
                        const int *d_labels, double *d_dist, double *d_colsum, double *d_pmean, hipStream_t stream);
int diarb_seed(const double *d_Z, long long ld, const int *d_rows, const diar::BatchJob *d_jobs, int n_jobs, const double *d_u,
               double *d_closest, double *d_tmp, double *d_centers, hipStream_t stream);
// one Lloyd iteration of every unfinished job (ints [n_jobs][33] is zeroed here), and the last pass (labels, d2, inertia)
int diarb_kmeans_step(const double *d_Z, long long ld, const int *d_rows, const diar::BatchJob *d_jobs, int n_jobs, int kmax,
                      long long max_n, int max_D, double *d_centers, diar::KmState *d_state, int *d_labels, double *d_d2,
                      int *d_ints, double *d_sums, int max_iter, hipStream_t stream);
int diarb_kmeans_last(const double *d_Z, long long ld, const int *d_rows, const diar::BatchJob *d_jobs, int n_jobs, int kmax,
                      long long max_n, const double *d_centers, const diar::KmState *d_state, int *d_labels, double *d_d2,
                      double *d_inertia, hipStream_t stream);
// tiles of the list, then the two reduction stages (records red1 -> stage, red2 -> S); max_bins: the widest clip
int diarb_pair_sums(const double *d_Z, long long ld, const int *d_rows, const diar::BatchClip *d_clips, const diar::BatchJob *d_jobs,
                    const diar::BatchTile *d_items, int n_items, const int *d_labels, const int *d_bintab, double *d_partial,
                    const diar::BatchRed *d_red1, int n_red1, double *d_stage, const diar::BatchRed *d_red2, int n_red2,
                    double *d_S, int max_bins, int workgroups, hipStream_t stream);
// kernels_lda.hpp (the LDA step of speaker diarization); classes are the runs off[c] .. off[c + 1] - 1 of windows (off [C + 1] on
// the device).  means [C][D] and std [D] (pooled within-class deviation, zeros replaced by 1); dev and sq [C][D] are scratch
int lda_class_stats(const double *d_X, long long ld, long long n, int D, const long long *d_off, long long C, double *d_means,
                    double *d_dev, double *d_sq, double *d_std, hipStream_t stream);
// G [D][D] = Xs^T Xs of Xs = (X - class mean) * rscale, in lda_gram_chunks(n) partials [D][D] each (scratch) added in chunk
// order; cls [n] is scratch
long long lda_gram_chunks(long long n);
int lda_within_gram(const double *d_X, long long ld, long long n, int D, const long long *d_off, long long C, const double *d_means,
                    const double *d_rscale, int *d_cls, double *d_partial, double *d_G, hipStream_t stream);
// Y [n_out][ldy] = ((X - xbar)^T S)^T, S [D][n_out]
int lda_project(const double *d_X, long long ld, long long n, int D, const double *d_xbar, const double *d_S, int n_out, double *d_Y,
                long long ldy, hipStream_t stream);

}  // namespace launch
}  // namespace paa
