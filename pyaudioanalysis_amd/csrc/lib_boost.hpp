// Fitting gradient-boosting classifiers on the device (audioTrainTest.train_gradient_boosting and the "gradientboosting" sweep of
// evaluate_classifier, audioTrainTest.py:181-199, :631-700): paa_boost_fit_splits_f64.  Every split is a job of n_estimators stages; a
// stage is two launches over the jobs that still have stages left -- boost_gradient_kernel (kernels_boost.hpp: the negative gradients
// of the stage and the loss of the stage before) and the kFriedman instance of tree_fit_kernel (kernels_treefit.hpp: one workgroup per
// (job, class) builds the stage's tree, takes the Newton step of every leaf and adds it to the leaf's rows of the raw predictions).
// The host queues all stages of a chunk of jobs without a synchronisation in between; the jobs are taken in the order of falling
// stage counts, so the jobs of a stage are a prefix of the chunk.  The test rows are scored by the boosted path of the predict
// kernels (kernels_forest.hpp) from the packed nodes; the trees cross to the host only when the caller asks for them.
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
    if (!X || !labels || !label_out || !train_off || !train_idx || !test_off || !test_idx || !mean || !std || !n_estimators || !tree_seed ||
        !init || !job_flags)
        return fail(PAA_ERR_ARG, "null argument");
    if (arrays && (!node_count || !children_left || !children_right || !feature || !threshold || !impurity || !n_node_samples ||
                   !weighted_n_node_samples || !missing_go_to_left || !value))
        return fail(PAA_ERR_ARG, "null argument");
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
    // per job the classes present in its training list, ascending, every row's place among them, and the job's place in the outputs
    struct Job {
        int n, k, k_out, n_est, cap;
        int64_t tree0, node0, score0, raw0;       // its first tree, node, loss and raw prediction in the caller's arrays
        size_t class0;
    };
    std::vector<Job> jobs(n_jobs);
    std::vector<int> row_label((size_t)n_t), job_class;
    int64_t trees = 0, nodes = 0, scores = 0, raws = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *tr = train_idx + train_off[j];
        const int64_t n = train_off[j + 1] - train_off[j];
        std::vector<int> classes;
        for (int64_t i = 0; i < n; ++i) classes.push_back(labels[tr[i]]);
        std::sort(classes.begin(), classes.end());
        classes.erase(std::unique(classes.begin(), classes.end()), classes.end());
        if ((rc = tree_job_check(j, n, (int)classes.size()))) return rc;
        const int k = (int)classes.size(), k_out = k == 2 ? 1 : k;
        if (k < 2) return fail(PAA_ERR_ARG, "job %d: its training rows hold one class; a boosted classifier needs two", j);
        if (k > max_classes) return fail(PAA_ERR_ARG, "max_classes = %d, job %d has %d classes", max_classes, j, k);
        if (n_estimators[j] < 1 || (int64_t)n_estimators[j] * k_out > kForestMaxTrees)
            return fail(PAA_ERR_ARG, "job %d: %d stages of %d trees: 1..%d trees are supported", j, n_estimators[j], k_out, kForestMaxTrees);
        for (int64_t i = 0; i < n; ++i)
            row_label[train_off[j] + i] = (int)(std::lower_bound(classes.begin(), classes.end(), labels[tr[i]]) - classes.begin());
        for (int c = 0; c < k_out; ++c)
            if (!std::isfinite(init[(size_t)j * max_classes + c])) return fail(PAA_ERR_ARG, "job %d: initial raw score %d is not finite", j, c);
        jobs[j] = {(int)n, k, k_out, n_estimators[j], boost_tree_cap((int)n, max_depth), trees, nodes, scores, raws, job_class.size()};
        job_class.insert(job_class.end(), classes.begin(), classes.end());
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
    const size_t per_node = sizeof(treefit::StackRec) + sizeof(forest::Node) + 8 + 4 + (arrays ? 41 : 0);
    auto job_bytes = [&](const Job &jb) {
        return (size_t)jb.n * n_dims * 4 + (size_t)jb.n_est * jb.k_out * jb.cap * per_node + (size_t)jb.n * jb.k_out * 16 + (size_t)jb.n * 8;
    };
    int chunks = 0;
    bool flagged = false;
    for (int o0 = 0; o0 < n_jobs && !flagged;) {
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
        std::vector<treefit::TreeJob> tjobs(nj);
        std::vector<boost::BoostJob> bjobs(nj);
        std::vector<int32_t> c_idx, c_label;
        std::vector<double> c_mean((size_t)nj * n_dims), c_std((size_t)nj * n_dims), c_init;
        std::vector<int64_t> job_node(nj + 1, 0), job_tree(nj + 1, 0), job_q(nj + 1, 0);
        std::vector<int> roots;
        int64_t x_words = 0, r_words = 0, c_scores = 0;
        int n_max = 0, k_all = 0;
        for (int jj = 0; jj < nj; ++jj) {
            const int j = order[o0 + jj];
            const Job &jb = jobs[j];
            tjobs[jj] = {(long long)c_idx.size(), (long long)x_words, jb.n, 1, jj, 0};
            bjobs[jj] = {(long long)c_idx.size(), (long long)r_words, (long long)c_scores, (long long)c_init.size(), jb.n, jb.k, jb.n_est, 0};
            c_idx.insert(c_idx.end(), train_idx + train_off[j], train_idx + train_off[j + 1]);
            c_label.insert(c_label.end(), row_label.begin() + train_off[j], row_label.begin() + train_off[j + 1]);
            std::copy(mean + (size_t)j * n_dims, mean + (size_t)(j + 1) * n_dims, c_mean.begin() + (size_t)jj * n_dims);
            std::copy(std + (size_t)j * n_dims, std + (size_t)(j + 1) * n_dims, c_std.begin() + (size_t)jj * n_dims);
            c_init.insert(c_init.end(), init + (size_t)j * max_classes, init + (size_t)j * max_classes + jb.k_out);
            for (int t = 0; t < jb.n_est * jb.k_out; ++t) roots.push_back(t * jb.cap);
            x_words += (int64_t)jb.n * n_dims;
            r_words += (int64_t)jb.n * jb.k_out;
            c_scores += jb.n_est;
            job_node[jj + 1] = job_node[jj] + (int64_t)jb.n_est * jb.k_out * jb.cap;
            job_tree[jj + 1] = job_tree[jj] + (int64_t)jb.n_est * jb.k_out;
            job_q[jj + 1] = job_q[jj] + (test_off[j + 1] - test_off[j]);
            n_max = std::max(n_max, jb.n);
            k_all = std::max(k_all, jb.k);
        }
        // the tasks stage after stage, within a stage job after job, class after class; a job's nodes stay together (stage-major)
        std::vector<treefit::TreeTask> tasks;
        std::vector<treefit::BoostTask> btasks;
        std::vector<int64_t> stage_first(s_max + 1, 0), task_tree;         // task_tree: the task's tree in the caller's order
        std::vector<int> stage_jobs(s_max + 2, 0);                          // jobs with at least s stages
        for (int s = 0; s < s_max; ++s) {
            stage_first[s] = (int64_t)tasks.size();
            for (int jj = 0; jj < nj && jobs[order[o0 + jj]].n_est > s; ++jj) {
                const Job &jb = jobs[order[o0 + jj]];
                for (int c = 0; c < jb.k_out; ++c) {
                    const int t = s * jb.k_out + c;
                    const long long node_off = (long long)(job_node[jj] + (int64_t)t * jb.cap);
                    tasks.push_back({-1, node_off, node_off, jj, jb.cap, t * jb.cap, (unsigned)tree_seed[jb.tree0 + t]});
                    btasks.push_back({bjobs[jj].r_off + (long long)c * jb.n, jb.k == 2 ? 1.0 : (double)(jb.k - 1) / (double)jb.k, jb.k == 2 ? 1 : c, 0});
                    task_tree.push_back(jb.tree0 + t);
                }
            }
        }
        stage_first[s_max] = (int64_t)tasks.size();
        for (int s = 0; s <= s_max + 1; ++s)
            for (int jj = 0; jj < nj; ++jj) stage_jobs[s] += jobs[order[o0 + jj]].n_est >= s;
        DevBlock in, work;
        BlockPart parts[] = {{tjobs.data(), tjobs.size() * sizeof(treefit::TreeJob), 8},
                             {tasks.data(), tasks.size() * sizeof(treefit::TreeTask), 8},
                             {btasks.data(), btasks.size() * sizeof(treefit::BoostTask), 8},
                             {bjobs.data(), bjobs.size() * sizeof(boost::BoostJob), 8},
                             {c_mean.data(), c_mean.size() * 8, 8},
                             {c_std.data(), c_std.size() * 8, 8},
                             {c_init.data(), c_init.size() * 8, 8},
                             {c_idx.data(), c_idx.size() * 4, 4},
                             {c_label.data(), c_label.size() * 4, 4},
                             {roots.data(), roots.size() * 4, 4}};
        if ((rc = block_upload(in, parts, 10, "the boosting jobs"))) return rc;
        const size_t tn = (size_t)c_nodes, n_tasks = tasks.size();
        const size_t b_x = up256((size_t)x_words * 4), b_flags = up256((size_t)nj * 4), b_stack = up256(tn * sizeof(treefit::StackRec)),
                     b_nodes = up256(tn * sizeof(forest::Node)), b_val = up256(tn * 8), b_cnt = up256(n_tasks * 4), b_i = up256(tn * 4),
                     b_d = up256(tn * 8), b_u = up256(tn), b_r = up256((size_t)r_words * 8), b_loss = up256((size_t)c_scores * 8);
        HIP_TRY(hipMalloc(&work.p, b_x + b_flags + b_stack + b_nodes + b_val + b_cnt + (arrays ? 4 * b_i + 3 * b_d + b_u : 0) + 2 * b_r + b_loss));
        char *p = (char *)work.p;
        treefit::TreeDev dev{};
        dev.n_dims = n_dims;
        dev.X = st.feats;
        dev.jobs = (const treefit::TreeJob *)parts[0].dev;
        const treefit::TreeTask *d_tasks = (const treefit::TreeTask *)parts[1].dev;
        const treefit::BoostTask *d_btasks = (const treefit::BoostTask *)parts[2].dev;
        dev.mean = (const double *)parts[4].dev;
        dev.scale = (const double *)parts[5].dev;
        const double *d_init = (const double *)parts[6].dev;
        dev.idx = (const int *)parts[7].dev;
        dev.label = (const int *)parts[8].dev;
        const int *d_roots = (const int *)parts[9].dev;
        dev.x32 = (float *)p;                   p += b_x;
        dev.flags = (int *)p;                   p += b_flags;
        dev.stack = (treefit::StackRec *)p;     p += b_stack;
        dev.nodes = (forest::Node *)p;          p += b_nodes;
        dev.value = (double *)p;                p += b_val;
        int *d_cnt = (int *)p;                  p += b_cnt;
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
        dev.raw = (double *)p;                  p += b_r;
        double *d_resid = (double *)p;          p += b_r;
        double *d_loss = (double *)p;
        dev.target = d_resid;
        dev.max_features = n_dims;
        dev.max_depth = max_depth;
        dev.learning_rate = learning_rate;
        boost::BoostDev bd{(const boost::BoostJob *)parts[3].dev, dev.label, d_init, dev.raw, d_resid, d_loss};
        LAUNCH_TRY("tree input", launch::tree_prep(dev, nj, n_max, cs()));
        std::vector<int> flags(nj, 0);
        HIP_TRY(hipMemcpyAsync(flags.data(), dev.flags, (size_t)nj * 4, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipStreamSynchronize(cs()));
        for (int jj = 0; jj < nj; ++jj) {
            job_flags[order[o0 + jj]] = flags[jj];
            flagged |= flags[jj] != 0;
        }
        if (flagged) break;                               // a NaN or an infinity in a training row: the caller reports it
        // the stages: two launches each, nothing waits in between
        for (int s = 0; s <= s_max; ++s) {
            LAUNCH_TRY("boosting gradient", launch::boost_gradient(bd, stage_jobs[s], s, cs()));
            if (s == s_max) break;
            dev.tasks = d_tasks + stage_first[s];
            dev.boost = d_btasks + stage_first[s];
            dev.node_count = d_cnt + stage_first[s];
            const int lrc = launch::tree_fit_boost(dev, (int)(stage_first[s + 1] - stage_first[s]), n_max, cs(), s == 0);
            if (lrc == -2) return fail(PAA_ERR_UNSUPPORTED, "the trees exceed the kernel's limits");
            if (lrc) return fail(PAA_ERR_HIP, "tree fit launch failed: %s", hipGetErrorString(hipGetLastError()));
        }
        // score every job's test rows: the traversal and reduction kernels of the predict path, boosted
        const int64_t q_chunk = job_q[nj];
        int64_t q_max = 0, leaf_max = 0, p_words = 0;
        for (int jj = 0; jj < nj; ++jj) {
            const Job &jb = jobs[order[o0 + jj]];
            const int64_t q = job_q[jj + 1] - job_q[jj];
            q_max = std::max(q_max, q);
            leaf_max = std::max(leaf_max, (int64_t)jb.n_est * jb.k_out * std::min<int64_t>(q, forest::kChunk));
            p_words += q * jb.k;
        }
        DevBlock score;
        std::vector<int32_t> h_label((size_t)q_chunk), h_test;
        std::vector<double> h_proba((size_t)p_words);
        if (q_chunk) {
            for (int jj = 0; jj < nj; ++jj) h_test.insert(h_test.end(), test_idx + test_off[order[o0 + jj]], test_idx + test_off[order[o0 + jj] + 1]);
            const size_t b_test = up256((size_t)q_chunk * 4), b_feats = up256((size_t)q_max * n_dims * 8), b_leaves = up256((size_t)leaf_max * 4),
                         b_raw = up256((size_t)q_max * k_all * 8), b_label = up256((size_t)q_chunk * 4), b_proba = up256((size_t)p_words * 8);
            HIP_TRY(hipMalloc(&score.p, b_test + b_feats + b_leaves + b_raw + b_label + b_proba));
            char *sp = (char *)score.p;
            int *d_test = (int *)sp;            sp += b_test;
            double *d_feats = (double *)sp;     sp += b_feats;
            int *d_leaves = (int *)sp;          sp += b_leaves;
            double *d_raw = (double *)sp;       sp += b_raw;
            int *d_label = (int *)sp;           sp += b_label;
            double *d_proba = (double *)sp;
            HIP_TRY(hipMemcpyAsync(d_test, h_test.data(), (size_t)q_chunk * 4, hipMemcpyHostToDevice, cs()));
            int64_t p_off = 0;
            for (int jj = 0; jj < nj; ++jj) {
                const Job &jb = jobs[order[o0 + jj]];
                const int64_t q = job_q[jj + 1] - job_q[jj];
                if (!q) continue;
                LAUNCH_TRY("scored row gather", launch::tree_gather(st.feats, n_dims, d_test + job_q[jj], q, d_feats, q, cs()));
                forest::ForestDev f{};
                f.nodes = dev.nodes + job_node[jj];
                f.roots = d_roots + job_tree[jj];
                f.leaf_values = dev.value + job_node[jj];
                f.init = d_init + bjobs[jj].init_off;
                f.n_trees = jb.n_est * jb.k_out;
                f.n_dims = n_dims;
                f.n_classes = jb.k;
                f.n_outputs = jb.k_out;
                f.boosted = 1;
                f.learning_rate = learning_rate;
                LAUNCH_TRY("tree-ensemble", launch::forest(f, d_feats, (long long)q, (long long)q, dev.mean + (size_t)jj * n_dims,
                                                           dev.scale + (size_t)jj * n_dims, d_leaves, d_label + job_q[jj], d_raw, d_proba + p_off, cs()));
                p_off += q * jb.k;
            }
            HIP_TRY(hipMemcpyAsync(h_label.data(), d_label, (size_t)q_chunk * 4, hipMemcpyDeviceToHost, cs()));
            if (proba) HIP_TRY(hipMemcpyAsync(h_proba.data(), d_proba, (size_t)p_words * 8, hipMemcpyDeviceToHost, cs()));
        }
        std::vector<double> h_loss(train_score ? (size_t)c_scores : 0), h_raw(train_raw ? (size_t)r_words : 0), h_res(train_resid ? (size_t)r_words : 0);
        if (train_resid) HIP_TRY(hipMemcpyAsync(h_res.data(), d_resid, (size_t)r_words * 8, hipMemcpyDeviceToHost, cs()));
        if (train_score) HIP_TRY(hipMemcpyAsync(h_loss.data(), d_loss, (size_t)c_scores * 8, hipMemcpyDeviceToHost, cs()));
        if (train_raw) HIP_TRY(hipMemcpyAsync(h_raw.data(), dev.raw, (size_t)r_words * 8, hipMemcpyDeviceToHost, cs()));
        std::vector<int32_t> h_cnt, h_i[4];
        std::vector<double> h_d[4];
        std::vector<uint8_t> h_u;
        if (arrays) {
            h_cnt.resize(n_tasks);
            HIP_TRY(hipMemcpyAsync(h_cnt.data(), d_cnt, n_tasks * 4, hipMemcpyDeviceToHost, cs()));
            const int *src_i[4] = {dev.children_left, dev.children_right, dev.feature, dev.n_node_samples};
            const double *src_d[4] = {dev.threshold, dev.impurity, dev.weighted_n_node_samples, dev.value};
            for (int a = 0; a < 4; ++a) {
                h_i[a].resize(tn);
                h_d[a].resize(tn);
                HIP_TRY(hipMemcpyAsync(h_i[a].data(), src_i[a], tn * 4, hipMemcpyDeviceToHost, cs()));
                HIP_TRY(hipMemcpyAsync(h_d[a].data(), src_d[a], tn * 8, hipMemcpyDeviceToHost, cs()));
            }
            h_u.resize(tn);
            HIP_TRY(hipMemcpyAsync(h_u.data(), dev.missing_go_to_left, tn, hipMemcpyDeviceToHost, cs()));
        }
        HIP_TRY(hipStreamSynchronize(cs()));
        // back to the caller's order
        int64_t p_off = 0;
        for (int jj = 0; jj < nj; ++jj) {
            const int j = order[o0 + jj];
            const Job &jb = jobs[j];
            for (int64_t q = 0; q < job_q[jj + 1] - job_q[jj]; ++q) {
                // a label is the position among the job's classes (-1: a test value is infinite in float32, -2: it is NaN)
                const int l = h_label[(size_t)(job_q[jj] + q)];
                label_out[test_off[j] + q] = l < 0 ? l : job_class[jb.class0 + l];
                if (proba)
                    for (int c = 0; c < jb.k; ++c) proba[(size_t)(test_off[j] + q) * max_classes + c] = h_proba[(size_t)(p_off + q * jb.k + c)];
            }
            p_off += (job_q[jj + 1] - job_q[jj]) * jb.k;
            if (train_score) std::copy(h_loss.begin() + bjobs[jj].loss_off, h_loss.begin() + bjobs[jj].loss_off + jb.n_est, train_score + jb.score0);
            if (train_raw)                                    // [k_out][n] on the device, [n][k_out] for the caller
                for (int c = 0; c < jb.k_out; ++c)
                    for (int i = 0; i < jb.n; ++i) train_raw[jb.raw0 + (int64_t)i * jb.k_out + c] = h_raw[(size_t)(bjobs[jj].r_off + (int64_t)c * jb.n + i)];
            if (train_resid)                                  // (the gradient kernel writes a job's residuals while it has stages left: these are its last stage's)
                for (int c = 0; c < jb.k_out; ++c)
                    for (int i = 0; i < jb.n; ++i) train_resid[jb.raw0 + (int64_t)i * jb.k_out + c] = h_res[(size_t)(bjobs[jj].r_off + (int64_t)c * jb.n + i)];
            if (arrays) {
                const size_t a = (size_t)job_node[jj], len = (size_t)(job_node[jj + 1] - job_node[jj]);
                int32_t *dst_i[4] = {children_left, children_right, feature, n_node_samples};
                double *dst_d[4] = {threshold, impurity, weighted_n_node_samples, value};
                for (int q = 0; q < 4; ++q) {
                    std::copy(h_i[q].begin() + a, h_i[q].begin() + a + len, dst_i[q] + jb.node0);
                    std::copy(h_d[q].begin() + a, h_d[q].begin() + a + len, dst_d[q] + jb.node0);
                }
                std::copy(h_u.begin() + a, h_u.begin() + a + len, missing_go_to_left + jb.node0);
            }
        }
        for (size_t t = 0; arrays && t < n_tasks; ++t) node_count[task_tree[t]] = h_cnt[t];
        o0 = o1;
    }
    if (n_chunks) *n_chunks = chunks;
    return PAA_OK;
}
