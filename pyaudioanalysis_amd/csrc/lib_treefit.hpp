// Fitting random forests and extra trees on the device (audioTrainTest.train_random_forest / train_extra_trees and the forest half
// of evaluate_classifier, audioTrainTest.py:158-219, :631-700): a batch of trees over index lists into ONE uploaded sample matrix,
// one workgroup per tree (paa_tree_fit_tasks_f64: the trees come back as scikit-learn's arrays), and the split sweep built on it
// (paa_forest_fit_splits_f64: the trees are fitted in chunks of bounded device scratch, every test row is scored by the
// traversal and reduction kernels of the predict path, no tree crosses to the host).  Kernels: kernels_treefit.hpp and
// kernels_forest.hpp (family_forest.hip).
// The regressor (train_random_forest_regression and the "randomforest" sweep of evaluate_regression, audioTrainTest.py:229-233,
// :774-855) goes the same two ways with targets in place of labels (paa_tree_fit_reg_tasks_f64, paa_forest_reg_fit_splits_f64):
// every job has ONE output, the trees are built by the squared-error instance of tree_fit_kernel with max_features = n_dims, and
// the sweep scores them as the averaged forest with one output.
// The pieces below are also the host path of the boosting sweep (lib_boost.hpp): JobClasses (a job's classes and its rows' places
// among them), TreeBatch (the device block of a batch of trees), TreeArrays (scikit-learn's arrays back on the host) and
// TreeScorer (row sets scored against a chunk's packed trees).
#pragma once

// the limits, for callers and tests: threads per workgroup, rows per job, classes, dims, the largest weight, MiB per chunk
extern "C" int paa_debug_tree_fit_geometry(int32_t *out6) {
    if (!out6) return fail(PAA_ERR_ARG, "null");
    launch::tree_fit_geometry(out6);
    return PAA_OK;
}

static int tree_params_check(int n_dims, int splitter) {
    if (n_dims < 1) return fail(PAA_ERR_ARG, "%d feature dimensions", n_dims);
    if (n_dims > treefit::kMaxDims) return fail(PAA_ERR_UNSUPPORTED, "%d feature dimensions: at most %d are supported", n_dims, treefit::kMaxDims);
    if (splitter != treefit::kBest && splitter != treefit::kRandom)
        return fail(PAA_ERR_ARG, "splitter %d: 0 (best, random forests) and 1 (random, extra trees) are supported", splitter);
    return PAA_OK;
}
static int tree_job_check(int j, int64_t n, int k) {
    if (n < 1) return fail(PAA_ERR_ARG, "job %d: no training rows", j);
    if (n > treefit::kMaxRows) return fail(PAA_ERR_UNSUPPORTED, "job %d: %lld training rows: at most %d per tree are supported", j, (long long)n, treefit::kMaxRows);
    if (k < 1) return fail(PAA_ERR_ARG, "job %d: %d classes", j, k);
    if (k > treefit::kMaxClasses) return fail(PAA_ERR_UNSUPPORTED, "job %d: %d classes: at most %d are supported", j, k, treefit::kMaxClasses);
    return PAA_OK;
}
// the targets of the rows idx [n] (idx null: the list itself) are finite
static int tree_target_check(const double *target, const int32_t *idx, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(target[idx ? idx[i] : i]))
            return fail(PAA_ERR_ARG, "target %lld is not finite", (long long)(idx ? idx[i] : i));
    return PAA_OK;
}
static int tree_seed_check(int t, int64_t seed) {
    if (seed < 0 || seed > 0xffffffffLL) return fail(PAA_ERR_ARG, "tree %d: seed %lld: a rand_r state is in 0 .. 2^32 - 1", t, (long long)seed);
    return PAA_OK;
}
// the weights of one tree over its job's n rows: 0 .. kMaxWeight, one of them positive; *in_bag: the rows with a positive weight
static int tree_weight_check(int t, const int32_t *w, int64_t n, int *in_bag) {
    int bag = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (w[i] < 0 || w[i] > treefit::kMaxWeight) return fail(PAA_ERR_ARG, "tree %d: weight %d of row %lld: 0 .. %d", t, w[i], (long long)i, treefit::kMaxWeight);
        bag += w[i] != 0;
    }
    if (!bag) return fail(PAA_ERR_ARG, "tree %d: every row has the weight 0", t);
    *in_bag = bag;
    return PAA_OK;
}
// a tree launch's return code as the library's
static int tree_launch_check(int lrc) {
    if (lrc == -2) return fail(PAA_ERR_UNSUPPORTED, "the trees exceed the kernel's limits");
    if (lrc) return fail(PAA_ERR_HIP, "tree fit launch failed: %s", hipGetErrorString(hipGetLastError()));
    return PAA_OK;
}

// Per job of a sweep the classes present in its training list, ascending, and every training row's place among them.  The jobs are
// added in order (their training lists follow each other), so a caller's own checks of job j fire before any check of job j + 1
struct JobClasses {
    std::vector<int> row_label, job_class;    // per training row of the sweep; the jobs' classes, job after job
    std::vector<size_t> off{0};               // job j's classes: job_class[off[j] .. off[j + 1] - 1]
    int k(int j) const { return (int)(off[j + 1] - off[j]); }
    const int *classes(int j) const { return job_class.data() + off[j]; }
    // the next job: the labels of its training rows tr [n]; runs tree_job_check
    int add(const int32_t *labels, const int32_t *tr, int64_t n) {
        std::vector<int> classes;
        for (int64_t i = 0; i < n; ++i) classes.push_back(labels[tr[i]]);
        std::sort(classes.begin(), classes.end());
        classes.erase(std::unique(classes.begin(), classes.end()), classes.end());
        int rc;
        if ((rc = tree_job_check((int)off.size() - 1, n, (int)classes.size()))) return rc;
        for (int64_t i = 0; i < n; ++i)
            row_label.push_back((int)(std::lower_bound(classes.begin(), classes.end(), labels[tr[i]]) - classes.begin()));
        job_class.insert(job_class.end(), classes.begin(), classes.end());
        off.push_back(job_class.size());
        return PAA_OK;
    }
};

// scikit-learn's arrays of a batch of trees on the host: node_count per task, value per value, the others per node
struct TreeArrays {
    int32_t *node_count, *children_left, *children_right, *feature;
    double *threshold, *impurity;
    int32_t *n_node_samples;
    double *weighted_n_node_samples;
    uint8_t *missing_go_to_left;
    double *value;
    bool complete() const {
        return node_count && children_left && children_right && feature && threshold && impurity && n_node_samples && weighted_n_node_samples &&
               missing_go_to_left && value;
    }
};

// One batch of trees on the device.  The caller fills jobs (off, n, k, stat; x_off is set here) and tasks (job, seed, w_off,
// cap = 2 in-bag rows - 1, node_rel; node_off / val_off are set here unless `placed`), uploads X and names the host arrays;
// prepare() uploads, allocates, makes the float32 copies and reads the flags back; when no job is flagged the caller launches --
// launch() for one launch over all tasks, the boosting sweep its stages.  With `target` (per job row) the trees are regression
// trees: every job's k is 1, the splitter the best one; `label` may stand beside it (the leaf step of a boosting stage reads it)
struct TreeBatch {
    std::vector<treefit::TreeJob> jobs;
    std::vector<treefit::TreeTask> tasks;
    std::vector<BlockPart> extra;             // the caller's own parts of the upload (their .dev after prepare())
    size_t extra_work = 0;                    // the caller's own bytes of the work block: at `spare` after prepare()
    char *spare = nullptr;
    const char *what = "the tree tasks";      // names the upload in its error message
    bool placed = false;                      // the caller has set node_off / val_off (a boosting chunk keeps a job's nodes together)
    std::vector<int> flags;                   // per job, after prepare()
    int64_t total_nodes = 0, total_values = 0;
    int inbag_max = 0, k_max = 0, n_max = 0;
    bool any_flag = false;
    int max_depth = -1;                       // >= 0 (with `target`): the trees of a boosting stage, Friedman's criterion under that depth
    DevBlock in, work;
    treefit::TreeDev dev{};
    // the offsets of the outputs: tree after tree, cap nodes and cap * k values each
    void layout() {
        int64_t x_off = 0;
        for (auto &j : jobs) {
            j.x_off = x_off;
            x_off += (int64_t)j.n * dev.n_dims;
            n_max = std::max(n_max, j.n);
            k_max = std::max(k_max, j.k);
        }
        x_words = x_off;
        total_nodes = total_values = 0;
        for (auto &t : tasks) {
            if (!placed) t.node_off = total_nodes, t.val_off = total_values;
            total_nodes += t.cap;
            total_values += (int64_t)t.cap * jobs[t.job].k;
            inbag_max = std::max(inbag_max, (t.cap + 1) / 2);
        }
    }
    int64_t x_words = 0;
    static constexpr size_t kArrayBytes = 4 * 4 + 3 * 8 + 1;      // of scikit-learn's arrays, per node (the values are counted apart)
    // device bytes of a batch with these totals (the sweeps cut their chunks by it)
    static size_t bytes(int64_t x_words, int64_t weights, int64_t nodes, int64_t values, bool arrays) {
        return (size_t)x_words * 4 + (size_t)weights * 4 + (size_t)nodes * (sizeof(treefit::StackRec) + sizeof(forest::Node) + (arrays ? kArrayBytes : 0)) +
               (size_t)values * 8;
    }
    // the trees of a classifier see sqrt(n_dims) features per split, those of a regressor all
    static int max_features(int n_dims, bool reg) { return reg ? n_dims : std::max(1, (int)std::sqrt((double)n_dims)); }
    int prepare(const double *d_X, const int32_t *idx, const int32_t *label, const double *target, int64_t rows, const int32_t *weight,
                int64_t n_weights, const double *mean, const double *std, int n_stats, int max_features, bool arrays) {
        const size_t sb = (size_t)n_stats * dev.n_dims * 8;
        const int32_t none = 0;
        std::vector<BlockPart> parts = {{jobs.data(), jobs.size() * sizeof(treefit::TreeJob), 8},
                                        {tasks.data(), tasks.size() * sizeof(treefit::TreeTask), 8},
                                        {mean, sb, 8},
                                        {std, sb, 8},
                                        {idx, (size_t)rows * 4, 4},
                                        {label, label ? (size_t)rows * 4 : 0, 4},
                                        {target, target ? (size_t)rows * 8 : 0, 8},
                                        {n_weights ? weight : &none, (size_t)std::max<int64_t>(n_weights, 1) * 4, 4}};
        const size_t own = parts.size();
        parts.insert(parts.end(), extra.begin(), extra.end());
        int rc;
        if ((rc = block_upload(in, parts.data(), (int)parts.size(), what))) return rc;
        std::copy(parts.begin() + own, parts.end(), extra.begin());
        const size_t n_t = tasks.size(), n_j = jobs.size(), tn = (size_t)total_nodes;
        const size_t b_x = up256((size_t)x_words * 4), b_flags = up256(n_j * 4), b_stack = up256(tn * sizeof(treefit::StackRec)),
                     b_nodes = up256(tn * sizeof(forest::Node)), b_val = up256((size_t)total_values * 8), b_cnt = up256(n_t * 4),
                     b_i = up256(tn * 4), b_d = up256(tn * 8), b_u = up256(tn);
        HIP_TRY(hipMalloc(&work.p, b_x + b_flags + b_stack + b_nodes + b_val + b_cnt + (arrays ? 4 * b_i + 3 * b_d + b_u : 0) + extra_work));
        char *p = (char *)work.p;
        dev.X = d_X;
        dev.jobs = (const treefit::TreeJob *)parts[0].dev;
        dev.tasks = (const treefit::TreeTask *)parts[1].dev;
        dev.mean = (const double *)parts[2].dev;
        dev.scale = (const double *)parts[3].dev;
        dev.idx = (const int *)parts[4].dev;
        dev.label = label ? (const int *)parts[5].dev : nullptr;
        dev.target = target ? (const double *)parts[6].dev : nullptr;
        dev.weight = (const int *)parts[7].dev;
        dev.x32 = (float *)p;                   p += b_x;
        dev.flags = (int *)p;                   p += b_flags;
        dev.stack = (treefit::StackRec *)p;     p += b_stack;
        dev.nodes = (forest::Node *)p;          p += b_nodes;
        dev.value = (double *)p;                p += b_val;
        dev.node_count = (int *)p;              p += b_cnt;
        if (arrays) {
            dev.children_left = (int *)p;       p += b_i;
            dev.children_right = (int *)p;      p += b_i;
            dev.feature = (int *)p;             p += b_i;
            dev.n_node_samples = (int *)p;      p += b_i;
            dev.threshold = (double *)p;        p += b_d;
            dev.impurity = (double *)p;         p += b_d;
            dev.weighted_n_node_samples = (double *)p;      p += b_d;
            dev.missing_go_to_left = (unsigned char *)p;    p += b_u;
        }
        spare = p;
        dev.max_features = max_features;
        dev.max_depth = max_depth;
        LAUNCH_TRY("tree input", launch::tree_prep(dev, (int)n_j, n_max, cs()));
        flags.assign(n_j, 0);
        HIP_TRY(hipMemcpyAsync(flags.data(), dev.flags, n_j * 4, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipStreamSynchronize(cs()));
        for (int f : flags) any_flag |= f != 0;   // a NaN or an infinity: nothing is fitted, the caller reports it
        return PAA_OK;
    }
    // every task in one launch
    int launch(int splitter) {
        const int n_t = (int)tasks.size();
        return tree_launch_check(dev.target ? (max_depth >= 0 ? launch::tree_fit_boost(dev, n_t, inbag_max, cs()) : launch::tree_fit_reg(dev, n_t, inbag_max, cs()))
                                            : launch::tree_fit(dev, n_t, splitter, inbag_max, k_max, cs()));
    }
    // queues the copies of the node counts and scikit-learn's arrays of the whole batch to the host (`arrays` of prepare())
    int read_arrays(const TreeArrays &h) const {
        const size_t tn = (size_t)total_nodes;
        HIP_TRY(hipMemcpyAsync(h.node_count, dev.node_count, tasks.size() * 4, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(h.children_left, dev.children_left, tn * 4, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(h.children_right, dev.children_right, tn * 4, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(h.feature, dev.feature, tn * 4, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(h.n_node_samples, dev.n_node_samples, tn * 4, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(h.threshold, dev.threshold, tn * 8, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(h.impurity, dev.impurity, tn * 8, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(h.weighted_n_node_samples, dev.weighted_n_node_samples, tn * 8, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(h.missing_go_to_left, dev.missing_go_to_left, tn, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(h.value, dev.value, (size_t)total_values * 8, hipMemcpyDeviceToHost, cs()));
        return PAA_OK;
    }
};

// One set of rows to score against the packed trees of a job of a TreeBatch, and where its results land on the host
struct ScoreRows {
    const int32_t *rows;          // the rows of X: host indices (uploaded by the scorer), or
    const int *d_rows;            // ... indices already on the device
    int64_t q;
    int64_t node0, val0;          // the job's first node and value in the batch
    const int *d_roots;           // [n_trees], node indices from node0
    int n_trees, n_classes, n_outputs;
    const double *d_init;         // boosted: the job's initial raw score [n_outputs]; null: an averaged forest
    double learning_rate;
    const double *d_mean, *d_scale;   // the job's rows of the standardisation
    // per row: label_out (classes[the label's place]; a negative label as it is), or without it flag |= 1 at a negative label (a
    // regression job: the test value is infinite in float32); proba_out [q][proba_ld], n_classes columns written.  Null: not wanted
    const int *classes;
    int32_t *label_out, *flag;
    double *proba_out;
    int proba_ld;
};
// Scores row sets with the traversal and reduction kernels of the predict path: queue() gathers, launches and queues the read-backs
// on the library stream, scatter() (after the caller's synchronisation) hands every set's results to its destinations
struct TreeScorer {
    std::vector<ScoreRows> sets;
    DevBlock block;
    std::vector<int32_t> h_label, h_rows;
    std::vector<double> h_proba;
    int queue(const double *d_X, int n_dims, const treefit::TreeDev &dev) {
        int64_t q_all = 0, p_all = 0, q_max = 0, leaf_max = 0, raw_max = 0;
        bool want_proba = false;
        for (const ScoreRows &s : sets) {
            q_all += s.q;
            p_all += s.q * s.n_classes;
            q_max = std::max(q_max, s.q);
            leaf_max = std::max(leaf_max, (int64_t)s.n_trees * std::min<int64_t>(s.q, forest::kChunk));
            raw_max = std::max(raw_max, s.q * s.n_outputs);
            want_proba |= s.proba_out != nullptr;
            if (s.rows) h_rows.insert(h_rows.end(), s.rows, s.rows + s.q);
        }
        if (!q_all) return PAA_OK;
        const size_t b_rows = up256(h_rows.size() * 4), b_feats = up256((size_t)q_max * n_dims * 8), b_leaves = up256((size_t)leaf_max * 4),
                     b_raw = up256((size_t)raw_max * 8), b_label = up256((size_t)q_all * 4), b_proba = up256((size_t)p_all * 8);
        HIP_TRY(hipMalloc(&block.p, b_rows + b_feats + b_leaves + b_raw + b_label + b_proba));
        char *p = (char *)block.p;
        int *d_rows = (int *)p;             p += b_rows;
        double *d_feats = (double *)p;      p += b_feats;
        int *d_leaves = (int *)p;           p += b_leaves;
        double *d_raw = (double *)p;        p += b_raw;
        int *d_label = (int *)p;            p += b_label;
        double *d_proba = (double *)p;
        if (!h_rows.empty()) HIP_TRY(hipMemcpyAsync(d_rows, h_rows.data(), h_rows.size() * 4, hipMemcpyHostToDevice, cs()));
        int64_t at = 0, at_p = 0, at_rows = 0;
        for (const ScoreRows &s : sets) {
            const int *rows = s.rows ? d_rows + at_rows : s.d_rows;
            if (s.rows) at_rows += s.q;
            if (!s.q) continue;
            LAUNCH_TRY("scored row gather", launch::tree_gather(d_X, n_dims, rows, s.q, d_feats, s.q, cs()));
            forest::ForestDev f{};
            f.nodes = dev.nodes + s.node0;
            f.roots = s.d_roots;
            f.leaf_values = dev.value + s.val0;
            f.init = s.d_init;
            f.n_trees = s.n_trees;
            f.n_dims = n_dims;
            f.n_classes = s.n_classes;
            f.n_outputs = s.n_outputs;
            f.boosted = s.d_init != nullptr;
            f.learning_rate = s.learning_rate;
            LAUNCH_TRY("tree-ensemble", launch::forest(f, d_feats, (long long)s.q, (long long)s.q, s.d_mean, s.d_scale, d_leaves, d_label + at, d_raw,
                                                       d_proba + at_p, cs()));
            at += s.q;
            at_p += s.q * s.n_classes;
        }
        h_label.resize((size_t)q_all);
        h_proba.resize((size_t)p_all);
        HIP_TRY(hipMemcpyAsync(h_label.data(), d_label, (size_t)q_all * 4, hipMemcpyDeviceToHost, cs()));
        if (want_proba) HIP_TRY(hipMemcpyAsync(h_proba.data(), d_proba, (size_t)p_all * 8, hipMemcpyDeviceToHost, cs()));
        return PAA_OK;
    }
    void scatter() const {
        int64_t at = 0, at_p = 0;
        for (const ScoreRows &s : sets) {
            for (int64_t r = 0; r < s.q; ++r) {
                // a label is the position among the job's classes (-1: a value is infinite in float32, -2: boosted and it is NaN)
                const int l = h_label[(size_t)(at + r)];
                if (s.label_out) s.label_out[r] = l < 0 ? l : s.classes[l];
                else if (l < 0 && s.flag) *s.flag |= 1;
                for (int c = 0; s.proba_out && c < s.n_classes; ++c) s.proba_out[r * s.proba_ld + c] = h_proba[(size_t)(at_p + r * s.n_classes + c)];
            }
            at += s.q;
            at_p += s.q * s.n_classes;
        }
    }
};

// The trees alone, classification (job_label, job_k) or regression (job_target): see paa_hip.h
static int tree_fit_tasks(const double *X, int64_t n_samples, int n_dims, int n_jobs, const int64_t *job_off, const int32_t *job_idx,
                          const int32_t *job_label, const int32_t *job_k, const double *job_target, const double *mean,
                          const double *std, int n_tasks, const int32_t *task_job, const int64_t *task_seed,
                          const int32_t *task_weight, int splitter, int max_depth, int64_t total_nodes, int64_t total_values, int32_t *job_flags,
                          const TreeArrays &out) {
    const bool reg = job_label == nullptr && job_k == nullptr;
    if (!X || !job_off || !job_idx || (reg ? !job_target : (!job_label || !job_k)) || !mean || !std || !task_job || !task_seed || !task_weight || !job_flags ||
        !out.complete())
        return fail(PAA_ERR_ARG, "null argument");
    int rc;
    if ((rc = sweep_samples_check(n_samples))) return rc;
    if ((rc = tree_params_check(n_dims, splitter))) return rc;
    if (n_jobs < 1 || n_jobs > 65535) return fail(PAA_ERR_ARG, "%d jobs: 1 .. 65535", n_jobs);
    if (n_tasks < 1) return fail(PAA_ERR_ARG, "no tasks");
    if ((rc = sweep_offsets_check(job_off, n_jobs, "job"))) return rc;
    const int64_t rows = job_off[n_jobs];
    TreeBatch b;
    b.dev.n_dims = n_dims;
    b.max_depth = max_depth;
    b.jobs.resize(n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t n = job_off[j + 1] - job_off[j];
        const int k = reg ? 1 : job_k[j];
        if ((rc = tree_job_check(j, n, k))) return rc;
        b.jobs[j] = {(long long)job_off[j], 0, (int)n, k, j, 0};
        for (int64_t i = job_off[j]; !reg && i < job_off[j + 1]; ++i)
            if (job_label[i] < 0 || job_label[i] >= k)
                return fail(PAA_ERR_ARG, "job %d: class index %d of row %lld: 0 .. %d", j, job_label[i], (long long)(i - job_off[j]), k - 1);
    }
    if (reg && (rc = tree_target_check(job_target, nullptr, rows))) return rc;
    if ((rc = sweep_index_check(job_idx, rows, n_samples, "row"))) return rc;
    b.tasks.resize(n_tasks);
    int64_t w_off = 0;
    for (int t = 0; t < n_tasks; ++t) {
        if (task_job[t] < 0 || task_job[t] >= n_jobs) return fail(PAA_ERR_ARG, "task %d: job %d of %d", t, task_job[t], n_jobs);
        if ((rc = tree_seed_check(t, task_seed[t]))) return rc;
        const int n = b.jobs[task_job[t]].n;
        int bag;
        if ((rc = tree_weight_check(t, task_weight + w_off, n, &bag))) return rc;
        b.tasks[t] = {(long long)w_off, 0, 0, task_job[t], 2 * bag - 1, 0, (unsigned)task_seed[t]};
        w_off += n;
    }
    b.layout();
    if (total_nodes != b.total_nodes || total_values != b.total_values)
        return fail(PAA_ERR_ARG, "total_nodes = %lld, total_values = %lld: the tasks make %lld nodes and %lld values", (long long)total_nodes,
                    (long long)total_values, (long long)b.total_nodes, (long long)b.total_values);
    if (b.total_nodes > 0x7fffffffLL) return fail(PAA_ERR_UNSUPPORTED, "too many nodes");
    if ((rc = ensure_init())) return rc;
    Staged st;                                        // X goes up once, through the lane's scratch
    if ((rc = stage(st, X, n_dims, n_samples, nullptr, nullptr, 0, {}))) return rc;
    if ((rc = b.prepare(st.feats, job_idx, job_label, job_target, rows, task_weight, w_off, mean, std, n_jobs, TreeBatch::max_features(n_dims, reg), true)))
        return rc;
    std::copy(b.flags.begin(), b.flags.end(), job_flags);
    if (b.any_flag) return PAA_OK;
    if ((rc = b.launch(splitter)) || (rc = b.read_arrays(out))) return rc;
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}
extern "C" int paa_tree_fit_tasks_f64(const double *X, int64_t n_samples, int n_dims, int n_jobs, const int64_t *job_off,
                                      const int32_t *job_idx, const int32_t *job_label, const int32_t *job_k, const double *mean,
                                      const double *std, int n_tasks, const int32_t *task_job, const int64_t *task_seed,
                                      const int32_t *task_weight, int splitter, int64_t total_nodes, int64_t total_values,
                                      int32_t *job_flags, int32_t *node_count, int32_t *children_left, int32_t *children_right,
                                      int32_t *feature, double *threshold, double *impurity, int32_t *n_node_samples,
                                      double *weighted_n_node_samples, uint8_t *missing_go_to_left, double *value) {
    if (!job_label || !job_k) return fail(PAA_ERR_ARG, "null argument");
    return tree_fit_tasks(X, n_samples, n_dims, n_jobs, job_off, job_idx, job_label, job_k, nullptr, mean, std, n_tasks, task_job, task_seed,
                          task_weight, splitter, -1, total_nodes, total_values, job_flags,
                          {node_count, children_left, children_right, feature, threshold, impurity, n_node_samples, weighted_n_node_samples,
                           missing_go_to_left, value});
}
extern "C" int paa_tree_fit_reg_tasks_f64(const double *X, int64_t n_samples, int n_dims, int n_jobs, const int64_t *job_off,
                                          const int32_t *job_idx, const double *job_target, const double *mean, const double *std,
                                          int n_tasks, const int32_t *task_job, const int64_t *task_seed, const int32_t *task_weight,
                                          int64_t total_nodes, int64_t total_values, int32_t *job_flags, int32_t *node_count,
                                          int32_t *children_left, int32_t *children_right, int32_t *feature, double *threshold,
                                          double *impurity, int32_t *n_node_samples, double *weighted_n_node_samples,
                                          uint8_t *missing_go_to_left, double *value) {
    return tree_fit_tasks(X, n_samples, n_dims, n_jobs, job_off, job_idx, nullptr, nullptr, job_target, mean, std, n_tasks, task_job,
                          task_seed, task_weight, treefit::kBest, -1, total_nodes, total_values, job_flags,
                          {node_count, children_left, children_right, feature, threshold, impurity, n_node_samples, weighted_n_node_samples,
                           missing_go_to_left, value});
}
extern "C" int paa_tree_fit_boost_tasks_f64(const double *X, int64_t n_samples, int n_dims, int n_jobs, const int64_t *job_off,
                                            const int32_t *job_idx, const double *job_target, const double *mean, const double *std,
                                            int n_tasks, const int32_t *task_job, const int64_t *task_seed, const int32_t *task_weight,
                                            int max_depth, int64_t total_nodes, int64_t total_values, int32_t *job_flags,
                                            int32_t *node_count, int32_t *children_left, int32_t *children_right, int32_t *feature,
                                            double *threshold, double *impurity, int32_t *n_node_samples,
                                            double *weighted_n_node_samples, uint8_t *missing_go_to_left, double *value) {
    if (max_depth < 1 || max_depth > treefit::kMaxRows) return fail(PAA_ERR_ARG, "max_depth = %d: 1 .. %d", max_depth, treefit::kMaxRows);
    return tree_fit_tasks(X, n_samples, n_dims, n_jobs, job_off, job_idx, nullptr, nullptr, job_target, mean, std, n_tasks, task_job,
                          task_seed, task_weight, treefit::kBest, max_depth, total_nodes, total_values, job_flags,
                          {node_count, children_left, children_right, feature, threshold, impurity, n_node_samples, weighted_n_node_samples,
                           missing_go_to_left, value});
}

// The forest half of audioTrainTest.evaluate_classifier (labels; label_out, proba) and the "randomforest" sweep of evaluate_regression
// (targets; pred, train_pred): every split a job of n_estimators trees; see paa_hip.h
static int forest_fit_splits(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, const double *targets, int n_jobs,
                             const int64_t *train_off, const int32_t *train_idx, const int64_t *test_off, const int32_t *test_idx,
                             const double *mean, const double *std, const int32_t *n_estimators, int splitter, const int64_t *tree_seed,
                             const int32_t *tree_weight, int32_t *label_out, double *proba, int max_classes, double *pred,
                             double *train_pred, int32_t *job_flags, int32_t *n_chunks) {
    // check
    const bool reg = targets != nullptr;
    if (!X || (reg ? !pred : (!labels || !label_out)) || !train_off || !train_idx || !test_off || !test_idx || !mean || !std || !n_estimators ||
        !tree_seed || !job_flags)
        return fail(PAA_ERR_ARG, "null argument");
    int rc;
    if ((rc = sweep_samples_check(n_samples))) return rc;
    if ((rc = tree_params_check(n_dims, splitter))) return rc;
    if ((rc = sweep_jobs_check(n_jobs, train_off, test_off))) return rc;
    const int64_t n_q = test_off[n_jobs], n_t = train_off[n_jobs];
    if ((rc = sweep_index_check(train_idx, n_t, n_samples, "train"))) return rc;
    if (reg && (rc = tree_target_check(targets, train_idx, n_t))) return rc;
    for (int64_t i = 0; !reg && i < n_t; ++i)
        if (labels[train_idx[i]] < 0) return fail(PAA_ERR_ARG, "training sample %d has the label %d: class indices are >= 0", train_idx[i], labels[train_idx[i]]);
    if ((rc = sweep_index_check(test_idx, n_q, n_samples, "test"))) return rc;
    JobClasses jc;                                    // (a regression job: one output, no classes)
    std::vector<double> row_target(reg ? (size_t)n_t : 0);
    for (int64_t i = 0; reg && i < n_t; ++i) row_target[i] = targets[train_idx[i]];
    std::vector<int64_t> first_tree(n_jobs + 1, 0), first_weight(n_jobs + 1, 0);
    std::vector<treefit::TreeJob> jobs(n_jobs);
    int k_all = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t n = train_off[j + 1] - train_off[j];
        if ((rc = reg ? tree_job_check(j, n, 1) : jc.add(labels, train_idx + train_off[j], n))) return rc;
        if (n_estimators[j] < 1 || n_estimators[j] > kForestMaxTrees)
            return fail(PAA_ERR_ARG, "job %d: %d trees: 1..%d are supported", j, n_estimators[j], kForestMaxTrees);
        jobs[j] = {(long long)train_off[j], 0, (int)n, reg ? 1 : jc.k(j), j, 0};
        k_all = std::max(k_all, jobs[j].k);
        first_tree[j + 1] = first_tree[j] + n_estimators[j];
        first_weight[j + 1] = first_weight[j] + (tree_weight ? (int64_t)n_estimators[j] * n : 0);
    }
    if (proba && max_classes < k_all) return fail(PAA_ERR_ARG, "max_classes = %d, a job has %d classes", max_classes, k_all);
    std::vector<int> caps((size_t)first_tree[n_jobs]);
    for (int j = 0; j < n_jobs; ++j)
        for (int e = 0; e < n_estimators[j]; ++e) {
            const int64_t t = first_tree[j] + e;
            if ((rc = tree_seed_check((int)t, tree_seed[t]))) return rc;
            int bag = jobs[j].n;
            if (tree_weight && (rc = tree_weight_check((int)t, tree_weight + first_weight[j] + (int64_t)e * jobs[j].n, jobs[j].n, &bag))) return rc;
            caps[t] = 2 * bag - 1;
        }
    if ((rc = ensure_init())) return rc;
    std::fill(job_flags, job_flags + n_jobs, 0);
    if (proba) std::fill(proba, proba + (size_t)n_q * max_classes, 0.0);      // zeros past a job's classes
    Staged st;                                        // X goes up once, through the lane's scratch
    if ((rc = stage(st, X, n_dims, n_samples, nullptr, nullptr, 0, {}))) return rc;
    // chunks of whole jobs within the scratch bound
    int chunks = 0;
    for (int j0 = 0; j0 < n_jobs;) {
        int j1 = j0;
        int64_t xw = 0, ww = 0, nodes = 0, values = 0;
        while (j1 < n_jobs) {
            int64_t jn = 0;
            for (int64_t t = first_tree[j1]; t < first_tree[j1 + 1]; ++t) jn += caps[t];
            const int64_t xw2 = xw + (int64_t)jobs[j1].n * n_dims, ww2 = ww + first_weight[j1 + 1] - first_weight[j1], nodes2 = nodes + jn,
                          values2 = values + jn * jobs[j1].k;
            if (j1 > j0 && (TreeBatch::bytes(xw2, ww2, nodes2, values2, false) > (size_t)treefit::kChunkBytes || nodes2 > 0x7fffffffLL)) break;
            xw = xw2, ww = ww2, nodes = nodes2, values = values2;
            ++j1;
        }
        if (nodes > 0x7fffffffLL) return fail(PAA_ERR_UNSUPPORTED, "job %d: too many nodes", j0);
        ++chunks;
        TreeBatch b;
        b.dev.n_dims = n_dims;
        std::vector<int> roots;
        std::vector<int64_t> job_node(j1 - j0 + 1, 0), job_val(j1 - j0 + 1, 0);
        for (int j = j0; j < j1; ++j) {
            treefit::TreeJob job = jobs[j];
            job.off -= train_off[j0];
            job.stat = j - j0;
            b.jobs.push_back(job);
            int64_t jn = 0;
            for (int e = 0; e < n_estimators[j]; ++e) {
                const int64_t t = first_tree[j] + e;
                const long long w_off = tree_weight ? (long long)(first_weight[j] - first_weight[j0] + (int64_t)e * job.n) : -1;
                b.tasks.push_back({w_off, 0, 0, j - j0, caps[t], (int)jn, (unsigned)tree_seed[t]});
                roots.push_back((int)jn);
                jn += caps[t];
            }
            job_node[j - j0 + 1] = job_node[j - j0] + jn;
            job_val[j - j0 + 1] = job_val[j - j0] + jn * job.k;
        }
        b.layout();
        b.extra = {{roots.data(), roots.size() * 4, 4}};
        if ((rc = b.prepare(st.feats, train_idx + train_off[j0], reg ? nullptr : jc.row_label.data() + train_off[j0],
                            reg ? row_target.data() + train_off[j0] : nullptr, train_off[j1] - train_off[j0],
                            tree_weight ? tree_weight + first_weight[j0] : nullptr, first_weight[j1] - first_weight[j0],
                            mean + (size_t)j0 * n_dims, std + (size_t)j0 * n_dims, j1 - j0, TreeBatch::max_features(n_dims, reg), false)))
            return rc;
        for (int j = j0; j < j1; ++j) job_flags[j] = b.flags[j - j0];
        if (b.any_flag) break;                            // a NaN or an infinity in a training row: the caller reports it
        if ((rc = b.launch(splitter))) return rc;
        // score every job's test rows with its trees.  A regression sweep that wants them scores every job's training rows too (the
        // chunk's uploaded train lists), behind the chunk's test rows
        TreeScorer sc;
        for (int pass = 0; pass < (reg && train_pred ? 2 : 1); ++pass)
            for (int j = j0; j < j1; ++j) {
                const treefit::TreeJob &job = b.jobs[j - j0];
                ScoreRows s{};
                if (pass) s.d_rows = b.dev.idx + job.off, s.q = job.n;
                else s.rows = test_idx + test_off[j], s.q = test_off[j + 1] - test_off[j];
                s.node0 = job_node[j - j0];
                s.val0 = job_val[j - j0];
                s.d_roots = (const int *)b.extra[0].dev + (first_tree[j] - first_tree[j0]);
                s.n_trees = n_estimators[j];
                s.n_classes = s.n_outputs = job.k;
                s.d_mean = b.dev.mean + (size_t)(j - j0) * n_dims;
                s.d_scale = b.dev.scale + (size_t)(j - j0) * n_dims;
                if (reg) {                                    // the averaged forest's one output is the width-1 probability
                    s.proba_out = pass ? train_pred + train_off[j] : pred + test_off[j];
                    s.proba_ld = 1;
                    s.flag = pass ? nullptr : job_flags + j;
                } else {
                    s.classes = jc.classes(j);
                    s.label_out = label_out + test_off[j];
                    s.proba_out = proba ? proba + (size_t)test_off[j] * max_classes : nullptr;
                    s.proba_ld = max_classes;
                }
                sc.sets.push_back(s);
            }
        if ((rc = sc.queue(st.feats, n_dims, b.dev))) return rc;
        HIP_TRY(hipStreamSynchronize(cs()));
        sc.scatter();
        j0 = j1;
    }
    if (n_chunks) *n_chunks = chunks;
    return PAA_OK;
}
extern "C" int paa_forest_fit_splits_f64(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs,
                                         const int64_t *train_off, const int32_t *train_idx, const int64_t *test_off,
                                         const int32_t *test_idx, const double *mean, const double *std, const int32_t *n_estimators,
                                         int splitter, const int64_t *tree_seed, const int32_t *tree_weight, int32_t *label_out,
                                         double *proba, int max_classes, int32_t *job_flags, int32_t *n_chunks) {
    if (!labels) return fail(PAA_ERR_ARG, "null argument");
    return forest_fit_splits(X, n_samples, n_dims, labels, nullptr, n_jobs, train_off, train_idx, test_off, test_idx, mean, std, n_estimators,
                             splitter, tree_seed, tree_weight, label_out, proba, max_classes, nullptr, nullptr, job_flags, n_chunks);
}
extern "C" int paa_forest_reg_fit_splits_f64(const double *X, int64_t n_samples, int n_dims, const double *targets, int n_jobs,
                                             const int64_t *train_off, const int32_t *train_idx, const int64_t *test_off,
                                             const int32_t *test_idx, const double *mean, const double *std,
                                             const int32_t *n_estimators, const int64_t *tree_seed, const int32_t *tree_weight,
                                             double *pred, double *train_pred, int32_t *job_flags, int32_t *n_chunks) {
    if (!targets) return fail(PAA_ERR_ARG, "null argument");
    return forest_fit_splits(X, n_samples, n_dims, nullptr, targets, n_jobs, train_off, train_idx, test_off, test_idx, mean, std,
                             n_estimators, treefit::kBest, tree_seed, tree_weight, nullptr, nullptr, 0, pred, train_pred, job_flags, n_chunks);
}
