// Fitting gradient-boosting classifiers on the device (audioTrainTest.train_gradient_boosting and the "gradientboosting" sweep of
// evaluate_classifier, audioTrainTest.py:181-199, :631-700): paa_boost_fit_splits_f64.  Every split is a job of n_estimators stages; a
// stage is two launches over the jobs that still have stages left -- boost_gradient_kernel (kernels_boost.hpp: the negative gradients
// of the stage and the loss of the stage before) and the kFriedman instance of tree_fit_kernel (kernels_treefit.hpp: one workgroup per
// (job, class) builds the stage's tree, takes the Newton step of every leaf and adds it to the leaf's rows of the raw predictions).
// The host queues all stages of a chunk of jobs without a synchronisation in between; the jobs are taken in the order of falling
// stage counts, so the jobs of a stage are a prefix of the chunk.  The test rows are scored by the boosted path of the predict
// kernels (kernels_forest.hpp) from the packed nodes; the trees cross to the host only when the caller asks for them.
// The classes of a job, the device block of a chunk, the scoring and the read-back of the arrays are lib_treefit.hpp's (JobClasses,
// TreeBatch, TreeScorer, TreeArrays); what is the sweep's own -- its rules, the order of the jobs, the stage tables and the way back
// to the caller's order -- is here.
#pragma once

constexpr int kBoostMaxDepth = 20;            // 2^(depth + 1) - 1 nodes per tree are laid out

// nodes laid out for a tree of n rows under max_depth
static inline int boost_tree_cap(int n, int max_depth) { return (int)std::min<int64_t>(2 * (int64_t)n - 1, ((int64_t)2 << max_depth) - 1); }

extern "C" int paa_boost_fit_splits_f64(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs,
                                        const int64_t *train_off, const int32_t *train_idx, const int64_t *test_off,
                                        const int32_t *test_idx, const double *mean, const double *std, const int32_t *n_estimators,
                                        const int64_t *tree_seed, const double *init, int max_classes, double learning_rate,
                                        int max_depth, int64_t chunk_bytes, int32_t *label_out, double *proba, double *train_score,
                                        double *train_raw, double *train_resid, int64_t total_nodes, int32_t *node_count, int32_t *children_left,
                                        int32_t *children_right, int32_t *feature, double *threshold, double *impurity,
                                        int32_t *n_node_samples, double *weighted_n_node_samples, uint8_t *missing_go_to_left,
                                        double *value, int32_t *job_flags, int32_t *n_chunks) {
    const bool arrays = total_nodes > 0;
    const TreeArrays out{node_count, children_left, children_right, feature, threshold, impurity, n_node_samples, weighted_n_node_samples,
                         missing_go_to_left, value};
    if (!X || !labels || !label_out || !train_off || !train_idx || !test_off || !test_idx || !mean || !std || !n_estimators || !tree_seed ||
        !init || !job_flags)
        return fail(PAA_ERR_ARG, "null argument");
    if (arrays && !out.complete()) return fail(PAA_ERR_ARG, "null argument");
    int rc;
    if ((rc = sweep_samples_check(n_samples))) return rc;
    if ((rc = tree_params_check(n_dims, treefit::kBest))) return rc;
    if (max_depth < 1 || max_depth > kBoostMaxDepth) return fail(PAA_ERR_ARG, "max_depth = %d: 1 .. %d", max_depth, kBoostMaxDepth);
    if (!(learning_rate > 0.0) || !std::isfinite(learning_rate)) return fail(PAA_ERR_ARG, "learning_rate = %g", learning_rate);
    if (max_classes < 2 || max_classes > treefit::kMaxClasses)
        return fail(max_classes > treefit::kMaxClasses ? PAA_ERR_UNSUPPORTED : PAA_ERR_ARG, "max_classes = %d: 2 .. %d", max_classes, treefit::kMaxClasses);
    if ((rc = sweep_jobs_check(n_jobs, train_off, test_off))) return rc;
    if (n_jobs > 65535) return fail(PAA_ERR_ARG, "%d jobs: 1 .. 65535", n_jobs);
    const int64_t n_q = test_off[n_jobs], n_t = train_off[n_jobs];
    if ((rc = sweep_index_check(train_idx, n_t, n_samples, "train"))) return rc;
    for (int64_t i = 0; i < n_t; ++i)
        if (labels[train_idx[i]] < 0) return fail(PAA_ERR_ARG, "training sample %d has the label %d: class indices are >= 0", train_idx[i], labels[train_idx[i]]);
    if ((rc = sweep_index_check(test_idx, n_q, n_samples, "test"))) return rc;
    // per job its classes (jc) and its place in the outputs
    struct Job {
        int n, k, k_out, n_est, cap;
        int64_t tree0, node0, score0, raw0;       // its first tree, node, loss and raw prediction in the caller's arrays
    };
    std::vector<Job> jobs(n_jobs);
    JobClasses jc;
    int64_t trees = 0, nodes = 0, scores = 0, raws = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t n = train_off[j + 1] - train_off[j];
        if ((rc = jc.add(labels, train_idx + train_off[j], n))) return rc;
        const int k = jc.k(j), k_out = k == 2 ? 1 : k;
        if (k < 2) return fail(PAA_ERR_ARG, "job %d: its training rows hold one class; a boosted classifier needs two", j);
        if (k > max_classes) return fail(PAA_ERR_ARG, "max_classes = %d, job %d has %d classes", max_classes, j, k);
        if (n_estimators[j] < 1 || (int64_t)n_estimators[j] * k_out > kForestMaxTrees)
            return fail(PAA_ERR_ARG, "job %d: %d stages of %d trees: 1..%d trees are supported", j, n_estimators[j], k_out, kForestMaxTrees);
        for (int c = 0; c < k_out; ++c)
            if (!std::isfinite(init[(size_t)j * max_classes + c])) return fail(PAA_ERR_ARG, "job %d: initial raw score %d is not finite", j, c);
        jobs[j] = {(int)n, k, k_out, n_estimators[j], boost_tree_cap((int)n, max_depth), trees, nodes, scores, raws};
        const int64_t jt = (int64_t)n_estimators[j] * k_out;
        for (int64_t t = 0; t < jt; ++t)
            if ((rc = tree_seed_check((int)(trees + t), tree_seed[trees + t]))) return rc;
        trees += jt;
        nodes += jt * jobs[j].cap;
        scores += n_estimators[j];
        raws += n * k_out;
    }
    if (arrays && total_nodes != nodes)
        return fail(PAA_ERR_ARG, "total_nodes = %lld: the jobs make %lld nodes", (long long)total_nodes, (long long)nodes);
    const size_t limit = chunk_bytes > 0 ? (size_t)std::min<int64_t>(chunk_bytes, treefit::kChunkBytes) : (size_t)treefit::kChunkBytes;
    if ((rc = ensure_init())) return rc;
    std::fill(job_flags, job_flags + n_jobs, 0);
    if (proba) std::fill(proba, proba + (size_t)n_q * max_classes, 0.0);      // zeros past a job's classes
    Staged st;                                        // X goes up once, through the lane's scratch
    if ((rc = stage(st, X, n_dims, n_samples, nullptr, nullptr, 0, {}))) return rc;
    // the jobs by falling stage counts (ties in the caller's order): the jobs of a stage are a prefix of every chunk
    std::vector<int> order(n_jobs);
    for (int j = 0; j < n_jobs; ++j) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return jobs[a].n_est > jobs[b].n_est; });
    // a job's share of a chunk: the batch of its trees (one value per node), a node count per node laid out, its raw predictions and
    // residuals, and 8 bytes per row
    auto job_bytes = [&](const Job &jb) {
        const int64_t jn = (int64_t)jb.n_est * jb.k_out * jb.cap;
        return TreeBatch::bytes((int64_t)jb.n * n_dims, 0, jn, jn, arrays) + (size_t)jn * 4 + (size_t)jb.n * jb.k_out * 16 + (size_t)jb.n * 8;
    };
    int chunks = 0;
    for (int o0 = 0; o0 < n_jobs;) {
        int o1 = o0;
        size_t bytes = 0;
        int64_t c_nodes = 0;
        while (o1 < n_jobs) {
            const Job &jb = jobs[order[o1]];
            const int64_t jn = (int64_t)jb.n_est * jb.k_out * jb.cap;
            if (o1 > o0 && (bytes + job_bytes(jb) > limit || c_nodes + jn > 0x7fffffffLL)) break;
            bytes += job_bytes(jb);
            c_nodes += jn;
            ++o1;
        }
        if (c_nodes > 0x7fffffffLL) return fail(PAA_ERR_UNSUPPORTED, "job %d: too many nodes", order[o0]);
        ++chunks;
        const int nj = o1 - o0, s_max = jobs[order[o0]].n_est;
        // the chunk's tables
        TreeBatch b;
        b.dev.n_dims = n_dims;
        b.max_depth = max_depth;
        b.what = "the boosting jobs";
        b.placed = true;
        std::vector<boost::BoostJob> bjobs(nj);
        std::vector<int32_t> c_idx, c_label;
        std::vector<double> c_mean((size_t)nj * n_dims), c_std((size_t)nj * n_dims), c_init;
        std::vector<int64_t> job_node(nj + 1, 0), job_tree(nj + 1, 0);
        std::vector<int> roots;
        int64_t r_words = 0, c_scores = 0;
        for (int jj = 0; jj < nj; ++jj) {
            const int j = order[o0 + jj];
            const Job &jb = jobs[j];
            b.jobs.push_back({(long long)c_idx.size(), 0, jb.n, 1, jj, 0});
            bjobs[jj] = {(long long)c_idx.size(), (long long)r_words, (long long)c_scores, (long long)c_init.size(), jb.n, jb.k, jb.n_est, 0};
            c_idx.insert(c_idx.end(), train_idx + train_off[j], train_idx + train_off[j + 1]);
            c_label.insert(c_label.end(), jc.row_label.begin() + train_off[j], jc.row_label.begin() + train_off[j + 1]);
            std::copy(mean + (size_t)j * n_dims, mean + (size_t)(j + 1) * n_dims, c_mean.begin() + (size_t)jj * n_dims);
            std::copy(std + (size_t)j * n_dims, std + (size_t)(j + 1) * n_dims, c_std.begin() + (size_t)jj * n_dims);
            c_init.insert(c_init.end(), init + (size_t)j * max_classes, init + (size_t)j * max_classes + jb.k_out);
            for (int t = 0; t < jb.n_est * jb.k_out; ++t) roots.push_back(t * jb.cap);
            r_words += (int64_t)jb.n * jb.k_out;
            c_scores += jb.n_est;
            job_node[jj + 1] = job_node[jj] + (int64_t)jb.n_est * jb.k_out * jb.cap;
            job_tree[jj + 1] = job_tree[jj] + (int64_t)jb.n_est * jb.k_out;
        }
        // the tasks stage after stage, within a stage job after job, class after class; a job's nodes stay together (stage-major)
        std::vector<treefit::BoostTask> btasks;
        std::vector<int64_t> stage_first(s_max + 1, 0), task_tree;         // task_tree: the task's tree in the caller's order
        std::vector<int> stage_jobs(s_max + 2, 0);                          // jobs with at least s stages
        for (int s = 0; s < s_max; ++s) {
            stage_first[s] = (int64_t)b.tasks.size();
            for (int jj = 0; jj < nj && jobs[order[o0 + jj]].n_est > s; ++jj) {
                const Job &jb = jobs[order[o0 + jj]];
                for (int c = 0; c < jb.k_out; ++c) {
                    const int t = s * jb.k_out + c;
                    const long long node_off = (long long)(job_node[jj] + (int64_t)t * jb.cap);
                    b.tasks.push_back({-1, node_off, node_off, jj, jb.cap, t * jb.cap, (unsigned)tree_seed[jb.tree0 + t]});
                    btasks.push_back({bjobs[jj].r_off + (long long)c * jb.n, jb.k == 2 ? 1.0 : (double)(jb.k - 1) / (double)jb.k, jb.k == 2 ? 1 : c, 0});
                    task_tree.push_back(jb.tree0 + t);
                }
            }
        }
        stage_first[s_max] = (int64_t)b.tasks.size();
        for (int s = 0; s <= s_max + 1; ++s)
            for (int jj = 0; jj < nj; ++jj) stage_jobs[s] += jobs[order[o0 + jj]].n_est >= s;
        b.layout();
        const size_t tn = (size_t)c_nodes, n_tasks = b.tasks.size(), b_r = up256((size_t)r_words * 8);
        b.extra = {{btasks.data(), btasks.size() * sizeof(treefit::BoostTask), 8},
                   {bjobs.data(), bjobs.size() * sizeof(boost::BoostJob), 8},
                   {c_init.data(), c_init.size() * 8, 8},
                   {roots.data(), roots.size() * 4, 4}};
        b.extra_work = 2 * b_r + up256((size_t)c_scores * 8);      // the raw predictions, the residuals, the losses
        if ((rc = b.prepare(st.feats, c_idx.data(), c_label.data(), nullptr, (int64_t)c_idx.size(), nullptr, 0, c_mean.data(), c_std.data(), nj,
                            n_dims, arrays)))
            return rc;
        for (int jj = 0; jj < nj; ++jj) job_flags[order[o0 + jj]] = b.flags[jj];
        if (b.any_flag) break;                            // a NaN or an infinity in a training row: the caller reports it
        const double *d_init = (const double *)b.extra[2].dev;
        double *d_resid = (double *)(b.spare + b_r), *d_loss = (double *)(b.spare + 2 * b_r);
        b.dev.raw = (double *)b.spare;
        b.dev.target = d_resid;
        b.dev.learning_rate = learning_rate;
        boost::BoostDev bd{(const boost::BoostJob *)b.extra[1].dev, b.dev.label, d_init, b.dev.raw, d_resid, d_loss};
        // the stages: two launches each, nothing waits in between.  `stage` is the batch as a stage's launch sees it: its first task on
        treefit::TreeDev stage = b.dev;
        for (int s = 0; s <= s_max; ++s) {
            LAUNCH_TRY("boosting gradient", launch::boost_gradient(bd, stage_jobs[s], s, cs()));
            if (s == s_max) break;
            stage.tasks = b.dev.tasks + stage_first[s];
            stage.boost = (const treefit::BoostTask *)b.extra[0].dev + stage_first[s];
            stage.node_count = b.dev.node_count + stage_first[s];
            if ((rc = tree_launch_check(launch::tree_fit_boost(stage, (int)(stage_first[s + 1] - stage_first[s]), b.n_max, cs(), s == 0)))) return rc;
        }
        // score every job's test rows: the boosted path of the predict kernels
        TreeScorer sc;
        for (int jj = 0; jj < nj; ++jj) {
            const int j = order[o0 + jj];
            const Job &jb = jobs[j];
            ScoreRows s{};
            s.rows = test_idx + test_off[j];
            s.q = test_off[j + 1] - test_off[j];
            s.node0 = s.val0 = job_node[jj];
            s.d_roots = (const int *)b.extra[3].dev + job_tree[jj];
            s.n_trees = jb.n_est * jb.k_out;
            s.n_classes = jb.k;
            s.n_outputs = jb.k_out;
            s.d_init = d_init + bjobs[jj].init_off;
            s.learning_rate = learning_rate;
            s.d_mean = b.dev.mean + (size_t)jj * n_dims;
            s.d_scale = b.dev.scale + (size_t)jj * n_dims;
            s.classes = jc.classes(j);
            s.label_out = label_out + test_off[j];
            s.proba_out = proba ? proba + (size_t)test_off[j] * max_classes : nullptr;
            s.proba_ld = max_classes;
            sc.sets.push_back(s);
        }
        if ((rc = sc.queue(st.feats, n_dims, b.dev))) return rc;
        std::vector<double> h_loss(train_score ? (size_t)c_scores : 0), h_raw(train_raw ? (size_t)r_words : 0), h_res(train_resid ? (size_t)r_words : 0);
        if (train_resid) HIP_TRY(hipMemcpyAsync(h_res.data(), d_resid, (size_t)r_words * 8, hipMemcpyDeviceToHost, cs()));
        if (train_score) HIP_TRY(hipMemcpyAsync(h_loss.data(), d_loss, (size_t)c_scores * 8, hipMemcpyDeviceToHost, cs()));
        if (train_raw) HIP_TRY(hipMemcpyAsync(h_raw.data(), b.dev.raw, (size_t)r_words * 8, hipMemcpyDeviceToHost, cs()));
        // the chunk's arrays, in the chunk's order
        std::vector<int32_t> h_i(arrays ? n_tasks + 4 * tn : 0);
        std::vector<double> h_d(arrays ? 4 * tn : 0);
        std::vector<uint8_t> h_u(arrays ? tn : 0);
        const TreeArrays got{h_i.data(), h_i.data() + n_tasks, h_i.data() + n_tasks + tn, h_i.data() + n_tasks + 2 * tn, h_d.data(), h_d.data() + tn,
                             h_i.data() + n_tasks + 3 * tn, h_d.data() + 2 * tn, h_u.data(), h_d.data() + 3 * tn};
        if (arrays && (rc = b.read_arrays(got))) return rc;
        HIP_TRY(hipStreamSynchronize(cs()));
        // back to the caller's order
        sc.scatter();
        for (int jj = 0; jj < nj; ++jj) {
            const Job &jb = jobs[order[o0 + jj]];
            if (train_score) std::copy(h_loss.begin() + bjobs[jj].loss_off, h_loss.begin() + bjobs[jj].loss_off + jb.n_est, train_score + jb.score0);
            if (train_raw)                                    // [k_out][n] on the device, [n][k_out] for the caller
                for (int c = 0; c < jb.k_out; ++c)
                    for (int i = 0; i < jb.n; ++i) train_raw[jb.raw0 + (int64_t)i * jb.k_out + c] = h_raw[(size_t)(bjobs[jj].r_off + (int64_t)c * jb.n + i)];
            if (train_resid)                                  // (the gradient kernel writes a job's residuals while it has stages left: these are its last stage's)
                for (int c = 0; c < jb.k_out; ++c)
                    for (int i = 0; i < jb.n; ++i) train_resid[jb.raw0 + (int64_t)i * jb.k_out + c] = h_res[(size_t)(bjobs[jj].r_off + (int64_t)c * jb.n + i)];
            if (arrays) {
                const size_t a = (size_t)job_node[jj], len = (size_t)(job_node[jj + 1] - job_node[jj]);
                auto put = [&](const auto *src, auto *dst) { std::copy(src + a, src + a + len, dst + jb.node0); };
                put(got.children_left, out.children_left), put(got.children_right, out.children_right), put(got.feature, out.feature);
                put(got.n_node_samples, out.n_node_samples), put(got.threshold, out.threshold), put(got.impurity, out.impurity);
                put(got.weighted_n_node_samples, out.weighted_n_node_samples), put(got.missing_go_to_left, out.missing_go_to_left);
                put(got.value, out.value);
            }
        }
        for (size_t t = 0; arrays && t < n_tasks; ++t) node_count[task_tree[t]] = got.node_count[t];
        o0 = o1;
    }
    if (n_chunks) *n_chunks = chunks;
    return PAA_OK;
}
