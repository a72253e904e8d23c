// The tree ensembles of audioTrainTest.classifier_wrapper (audioTrainTest.py:84-93) -- scikit-learn's RandomForestClassifier,
// ExtraTreesClassifier (averaged forests) and GradientBoostingClassifier (boosted sums) -- and the RandomForestRegressor of
// regression_wrapper (:96-111; an averaged forest with one output, its prediction in the width-1 proba) -- behind a handle,
// host-buffer and device-buffer predict calls.  Kernels: kernels_forest.hpp (family_forest.hip).
// paa_forest_create takes scikit-learn's raw per-tree arrays, validates every index before anything reaches the device, and
// re-lays each tree in preorder (left child = next node, 16-byte nodes, leaf values in their own array).
#pragma once

struct PaaForest {
    forest::ForestDev dev{};
    DevBlock block;               // nodes, leaf values, init, roots
};
static std::mutex g_forest_mu;
constexpr int kForestMaxTrees = 200000;       // grid limit of the traversal kernel (4 trees per workgroup row)

extern "C" int paa_forest_create(int kind, int n_trees, const int64_t *node_offsets, const int64_t *children_left,
                                 const int64_t *children_right, const int64_t *feature, const double *threshold,
                                 const uint8_t *missing_go_to_left, const double *value, int n_classes, int n_dims,
                                 double learning_rate, const double *init, void **out_handle) {
    if (!out_handle) return fail(PAA_ERR_ARG, "null handle pointer");
    *out_handle = nullptr;
    if (!node_offsets || !children_left || !children_right || !feature || !threshold || !value)
        return fail(PAA_ERR_ARG, "null argument");
    if (kind != PAA_FOREST_AVERAGED && kind != PAA_FOREST_BOOSTED && kind != PAA_FOREST_REGRESSOR)
        return fail(PAA_ERR_ARG, "ensemble kind %d", kind);
    // a regressor is an averaged forest with ONE output (RandomForestRegressor, audioTrainTest.py:229-233): value [nodes]
    if (kind == PAA_FOREST_REGRESSOR ? n_classes != 1 : (n_classes < 2 || n_classes > forest::kMaxClasses))
        return kind == PAA_FOREST_REGRESSOR ? fail(PAA_ERR_ARG, "a regressor has one output, not %d", n_classes)
                                            : fail(PAA_ERR_ARG, "%d classes: 2..%d are supported", n_classes, forest::kMaxClasses);
    if (n_dims < 1 || n_dims > forest::kMaxDims)
        return fail(PAA_ERR_ARG, "%d feature dimensions: 1..%d are supported", n_dims, forest::kMaxDims);
    if (n_trees < 1 || n_trees > kForestMaxTrees) return fail(PAA_ERR_ARG, "%d trees: 1..%d are supported", n_trees, kForestMaxTrees);
    const bool boosted = kind == PAA_FOREST_BOOSTED;
    const int n_outputs = boosted ? (n_classes == 2 ? 1 : n_classes) : n_classes;
    const int width = boosted ? 1 : n_classes;            // values per node in `value`
    if (boosted && n_trees % n_outputs)
        return fail(PAA_ERR_ARG, "%d trees are not whole stages of %d outputs", n_trees, n_outputs);
    if (boosted) {
        if (!init) return fail(PAA_ERR_ARG, "a boosted model needs its init scores");
        if (!std::isfinite(learning_rate)) return fail(PAA_ERR_ARG, "learning rate is not finite");
        for (int k = 0; k < n_outputs; ++k)
            if (!std::isfinite(init[k])) return fail(PAA_ERR_ARG, "init score %d is not finite", k);
    }
    if (node_offsets[0] != 0) return fail(PAA_ERR_ARG, "node offsets must start at 0");
    for (int t = 0; t < n_trees; ++t)
        if (node_offsets[t + 1] <= node_offsets[t]) return fail(PAA_ERR_ARG, "tree %d has no nodes", t);
    const int64_t total = node_offsets[n_trees];
    if (total >= 0x7fffffffLL) return fail(PAA_ERR_ARG, "%lld nodes: fewer than 2^31 are supported", (long long)total);

    // preorder packing; every node of a tree must be reached exactly once from its root
    std::vector<forest::Node> nodes((size_t)total);
    std::vector<int> roots(n_trees);
    std::vector<double> leaf_values;
    std::vector<char> seen((size_t)total, 0);
    std::vector<std::pair<int64_t, int64_t>> stack;            // (original node, packed parent whose right child it is, or -1)
    int64_t out = 0, n_leaves = 0;
    for (int t = 0; t < n_trees; ++t) {
        const int64_t base = node_offsets[t], size = node_offsets[t + 1] - base;
        roots[t] = (int)out;
        stack.assign(1, {0, -1});
        while (!stack.empty()) {
            const int64_t i = stack.back().first, parent = stack.back().second;
            stack.pop_back();
            const int64_t g = base + i;
            if (seen[g]) return fail(PAA_ERR_ARG, "tree %d: node %lld is reached twice (a cycle or a shared child)", t, (long long)i);
            seen[g] = 1;
            if (parent >= 0) nodes[parent].next = (int)out;
            forest::Node &nd = nodes[out];
            const int64_t l = children_left[g], r = children_right[g];
            if (l == -1 && r == -1) {
                nd.threshold = 0.0;
                nd.meta = forest::kLeaf;
                nd.next = (int)n_leaves++;
                leaf_values.insert(leaf_values.end(), value + g * width, value + (g + 1) * width);
            } else {
                if (l < 0 || l >= size || r < 0 || r >= size)
                    return fail(PAA_ERR_ARG, "tree %d: node %lld has children %lld / %lld outside 0..%lld", t, (long long)i,
                                (long long)l, (long long)r, (long long)(size - 1));
                const int64_t f = feature[g];
                if (f < 0 || f >= n_dims)
                    return fail(PAA_ERR_ARG, "tree %d: node %lld splits on feature %lld of %d", t, (long long)i, (long long)f, n_dims);
                nd.threshold = threshold[g];
                nd.meta = (int)f | (missing_go_to_left && missing_go_to_left[g] ? forest::kMissingLeft : 0);
                nd.next = -1;
                stack.push_back({r, out});                    // popped after the whole left subtree
                stack.push_back({l, -1});                     // popped next: packed at out + 1
            }
            ++out;
        }
        if (out - roots[t] != size)
            return fail(PAA_ERR_ARG, "tree %d: %lld of its %lld nodes are not reached from the root", t,
                        (long long)(size - (out - roots[t])), (long long)size);
    }

    int rc = ensure_init();
    if (rc) return rc;
    std::vector<double> init_v(n_outputs, 0.0);
    if (boosted) std::copy(init, init + n_outputs, init_v.begin());
    std::unique_ptr<PaaForest> h(new PaaForest());
    BlockPart parts[] = {{nodes.data(), (size_t)total * sizeof(forest::Node), sizeof(forest::Node)},
                         {leaf_values.data(), leaf_values.size() * 8, 8}, {init_v.data(), (size_t)n_outputs * 8, 8},
                         {roots.data(), (size_t)n_trees * sizeof(int), 4}};
    if ((rc = block_upload(h->block, parts, 4, "the tree ensemble"))) return rc;
    h->dev.nodes = (const forest::Node *)parts[0].dev;
    h->dev.leaf_values = (const double *)parts[1].dev;
    h->dev.init = (const double *)parts[2].dev;
    h->dev.roots = (const int *)parts[3].dev;
    h->dev.n_trees = n_trees;
    h->dev.n_dims = n_dims;
    h->dev.n_classes = n_classes;
    h->dev.n_outputs = n_outputs;
    h->dev.boosted = boosted;
    h->dev.learning_rate = boosted ? learning_rate : 0.0;
    *out_handle = h.release();
    return PAA_OK;
}

extern "C" int paa_forest_destroy(void *handle) { return model_destroy((PaaForest *)handle); }

extern "C" int paa_forest_num_classes(const void *handle) {
    return handle ? ((const PaaForest *)handle)->dev.n_classes : fail(PAA_ERR_ARG, "null handle");
}

static size_t forest_leaf_bytes(const forest::ForestDev &m, int64_t n_vec) {
    return (size_t)m.n_trees * (size_t)std::min<int64_t>(n_vec, forest::kChunk) * sizeof(int);
}

extern "C" int paa_forest_dev_predict_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                                          const double *d_mean, const double *d_std, int32_t *d_label_index, double *d_proba,
                                          double *d_raw) {
    int rc = model_check<PaaForest>(handle, n_dims, ld, n_vec, 0);
    if (rc) return rc;
    if (!d_feats || !d_mean || !d_std || !d_label_index || !d_proba) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    const forest::ForestDev &m = ((const PaaForest *)handle)->dev;
    std::lock_guard<std::mutex> lk(g_forest_mu);
    const size_t lb = up256(forest_leaf_bytes(m, n_vec));
    {
        std::lock_guard<std::mutex> lk2(g_mu);
        if ((rc = scratch_reserve(g_forest_scratch, lb + (d_raw ? 0 : (size_t)n_vec * m.n_outputs * 8)))) return rc;
    }
    double *raw = d_raw ? d_raw : (double *)((char *)g_forest_scratch.p + lb);
    LAUNCH_TRY("tree-ensemble", launch::forest(m, d_feats, (long long)ld, (long long)n_vec, d_mean, d_std, (int *)g_forest_scratch.p,
                                               d_label_index, raw, d_proba, cs()));
    return PAA_OK;
}

extern "C" int paa_forest_predict_f64(const void *handle, const double *feats, int n_dims, int64_t ld, int64_t n_vec,
                                      const double *mean, const double *std, int32_t *label_index, double *proba, double *raw) {
    int rc = model_check<PaaForest>(handle, n_dims, ld, n_vec, 0);
    if (rc) return rc;
    if (!feats || !mean || !std || !label_index || !proba) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    const forest::ForestDev &m = ((const PaaForest *)handle)->dev;
    const size_t lb = up256(forest_leaf_bytes(m, n_vec)), rwb = (size_t)n_vec * m.n_outputs * 8;
    Staged st;
    if ((rc = stage(st, feats, n_dims, ld, mean, std, lb + rwb,
                    {{label_index, (size_t)n_vec * 4}, {proba, (size_t)n_vec * m.n_classes * 8}})))
        return rc;
    double *d_raw = (double *)((char *)st.mid + lb);        // the raw scores live behind the leaf slots, not among the outputs
    LAUNCH_TRY("tree-ensemble", launch::forest(m, st.feats, (long long)ld, (long long)n_vec, st.mean, st.std, (int *)st.mid,
                                               (int32_t *)st.out[0], d_raw, (double *)st.out[1], cs()));
    if (raw) HIP_TRY(hipMemcpyAsync(raw, d_raw, rwb, hipMemcpyDeviceToHost, cs()));
    return finish(st);
}
