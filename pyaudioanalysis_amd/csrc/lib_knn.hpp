// The k-nearest-neighbour classifier of audioTrainTest.Knn (audioTrainTest.py:33-49) for the shipped knn_* models: an
// uploaded model behind a handle, host-buffer and device-buffer predict calls.  Kernel: kernels_knn.hpp (family_knn.hip).
#pragma once

struct PaaKnn {
    knn::KnnDev dev{};
    DevBlock block;               // training rows, then labels
};

extern "C" int paa_knn_create(const double *train, const int32_t *labels, int n_train, int n_dims, int n_classes, int k,
                              void **out_handle) {
    if (!out_handle) return fail(PAA_ERR_ARG, "null handle pointer");
    *out_handle = nullptr;
    if (!train || !labels) return fail(PAA_ERR_ARG, "null argument");
    if (k < 1 || k > knn::kMaxK) return fail(PAA_ERR_ARG, "k = %d neighbours: 1..%d are supported", k, knn::kMaxK);
    if (n_classes < 1 || n_classes > knn::kMaxClasses)
        return fail(PAA_ERR_ARG, "%d classes: 1..%d are supported", n_classes, knn::kMaxClasses);
    if (n_dims < 1 || n_dims > knn::kMaxDims) return fail(PAA_ERR_ARG, "%d feature dimensions: 1..%d are supported", n_dims, knn::kMaxDims);
    if (n_train < 1) return fail(PAA_ERR_ARG, "no training vectors");
    int rc = ensure_init();
    if (rc) return rc;
    std::unique_ptr<PaaKnn> h(new PaaKnn());
    BlockPart parts[] = {{train, (size_t)n_train * n_dims * 8, 8}, {labels, (size_t)n_train * sizeof(int), 4}};
    if ((rc = block_upload(h->block, parts, 2, "the kNN model"))) return rc;
    h->dev.train = (const double *)parts[0].dev;
    h->dev.labels = (const int *)parts[1].dev;
    h->dev.n_train = n_train;
    h->dev.n_dims = n_dims;
    h->dev.n_classes = n_classes;
    h->dev.k = k;
    *out_handle = h.release();
    return PAA_OK;
}

extern "C" int paa_knn_destroy(void *handle) { return model_destroy((PaaKnn *)handle); }

extern "C" int paa_knn_num_classes(const void *handle) {
    return handle ? ((const PaaKnn *)handle)->dev.n_classes : fail(PAA_ERR_ARG, "null handle");
}

constexpr int64_t kKnnMaxVec = 0x7fffffffLL * knn::kQueriesPerBlock;      // grid limit

extern "C" int paa_knn_dev_predict_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                                       const double *d_mean, const double *d_std, int32_t *d_label_index, double *d_proba,
                                       int32_t *d_neighbors) {
    int rc = model_check<PaaKnn>(handle, n_dims, ld, n_vec, kKnnMaxVec);
    if (rc) return rc;
    if (!d_feats || !d_mean || !d_std || !d_label_index || !d_proba) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    LAUNCH_TRY("kNN", launch::knn(((const PaaKnn *)handle)->dev, d_feats, (long long)ld, (long long)n_vec, d_mean, d_std,
                                  d_label_index, d_proba, d_neighbors, cs()));
    return PAA_OK;
}

extern "C" int paa_knn_predict_f64(const void *handle, const double *feats, int n_dims, int64_t ld, int64_t n_vec,
                                   const double *mean, const double *std, int32_t *label_index, double *proba,
                                   int32_t *neighbors) {
    int rc = model_check<PaaKnn>(handle, n_dims, ld, n_vec, kKnnMaxVec);
    if (rc) return rc;
    if (!feats || !mean || !std || !label_index || !proba) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    const knn::KnnDev &m = ((const PaaKnn *)handle)->dev;
    Staged st;
    if ((rc = stage(st, feats, n_dims, ld, mean, std, 0,
                    {{label_index, (size_t)n_vec * 4}, {proba, (size_t)n_vec * m.n_classes * 8}, {neighbors, (size_t)n_vec * m.k * 4}})))
        return rc;
    LAUNCH_TRY("kNN", launch::knn(m, st.feats, (long long)ld, (long long)n_vec, st.mean, st.std, (int32_t *)st.out[0],
                                  (double *)st.out[1], (int32_t *)st.out[2], cs()));
    return finish(st);
}

// queries per workgroup, training rows per LDS tile, rows per step, the number of K instances and the instances (for the edge tests)
extern "C" int paa_debug_knn_split_geometry(int32_t *out10) {
    if (!out10) return fail(PAA_ERR_ARG, "null");
    launch::knn_split_geometry(out10);
    return PAA_OK;
}

// The kNN half of audioTrainTest.evaluate_classifier (audioTrainTest.py:631-700): every (parameter value, experiment) split as a
// job of index lists over ONE uploaded sample matrix, all jobs in one launch (knn_split_kernel).
extern "C" int paa_knn_splits_f64(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs,
                                  const int64_t *train_off, const int32_t *train_idx, const int64_t *test_off,
                                  const int32_t *test_idx, const double *mean, const double *std, const int32_t *k,
                                  const int32_t *n_classes, int max_classes, int32_t *label_out, double *proba_out,
                                  int32_t *neighbors_out) {
    if (!X || !labels || !train_off || !train_idx || !test_off || !test_idx || !mean || !std || !k || !n_classes || !label_out)
        return fail(PAA_ERR_ARG, "null argument");
    int rc;
    if ((rc = sweep_samples_check(n_samples))) return rc;
    if (n_dims < 1 || n_dims > knn::kMaxDims) return fail(PAA_ERR_ARG, "%d feature dimensions: 1..%d are supported", n_dims, knn::kMaxDims);
    if (max_classes < 1 || max_classes > knn::kMaxClasses)
        return fail(PAA_ERR_ARG, "%d classes: 1..%d are supported", max_classes, knn::kMaxClasses);
    if ((rc = sweep_jobs_check(n_jobs, train_off, test_off))) return rc;
    const int64_t n_q = test_off[n_jobs], n_t = train_off[n_jobs];
    int k_max = 0;
    for (int j = 0; j < n_jobs; ++j) {
        if (k[j] < 1 || k[j] > knn::kMaxK) return fail(PAA_ERR_ARG, "job %d: k = %d neighbours: 1..%d are supported", j, k[j], knn::kMaxK);
        if (n_classes[j] < 1 || n_classes[j] > max_classes)
            return fail(PAA_ERR_ARG, "job %d: %d classes: 1..%d (max_classes)", j, n_classes[j], max_classes);
        if (train_off[j + 1] == train_off[j]) return fail(PAA_ERR_ARG, "job %d: no training vectors", j);
        k_max = std::max(k_max, (int)k[j]);
    }
    if ((rc = sweep_index_check(train_idx, n_t, n_samples, "train"))) return rc;
    if ((rc = sweep_index_check(test_idx, n_q, n_samples, "test"))) return rc;
    if (n_q == 0) return PAA_OK;                      // every test list empty: nothing to classify
    if ((rc = ensure_init())) return rc;
    const std::vector<knn::SplitBlock> blocks = sweep_blocks(test_off, n_jobs, knn::kQueriesPerBlock);
    const int k_launch = launch::knn_split_k_launch(k_max);
    const size_t sb = (size_t)n_jobs * n_dims * 8;
    DevBlock block;                                   // the job tables: freed on return
    BlockPart parts[] = {{labels, (size_t)n_samples * 4, 4},     {train_off, (size_t)(n_jobs + 1) * 8, 8},
                         {test_off, (size_t)(n_jobs + 1) * 8, 8}, {train_idx, (size_t)n_t * 4, 4},
                         {test_idx, (size_t)n_q * 4, 4},          {mean, sb, 8},
                         {std, sb, 8},                            {k, (size_t)n_jobs * 4, 4},
                         {n_classes, (size_t)n_jobs * 4, 4},      {blocks.data(), blocks.size() * sizeof(knn::SplitBlock), 8}};
    if ((rc = block_upload(block, parts, 10, "the kNN split jobs"))) return rc;
    Staged st;                                        // X goes up once, through the lane's scratch
    if ((rc = stage(st, X, n_dims, n_samples, nullptr, nullptr, 0,
                    {{label_out, (size_t)n_q * 4}, {proba_out, (size_t)n_q * max_classes * 8}, {neighbors_out, (size_t)n_q * k_launch * 4}})))
        return rc;
    knn::KnnSplitDev m{};
    m.X = st.feats;
    m.labels = (const int *)parts[0].dev;
    m.train_off = (const long long *)parts[1].dev;
    m.test_off = (const long long *)parts[2].dev;
    m.train_idx = (const int *)parts[3].dev;
    m.test_idx = (const int *)parts[4].dev;
    m.mean = (const double *)parts[5].dev;
    m.scale = (const double *)parts[6].dev;
    m.k = (const int *)parts[7].dev;
    m.n_classes = (const int *)parts[8].dev;
    m.blocks = (const knn::SplitBlock *)parts[9].dev;
    m.n_dims = n_dims;
    m.max_classes = max_classes;
    LAUNCH_TRY("kNN split", launch::knn_split(m, (long long)blocks.size(), k_max, (int32_t *)st.out[0], (double *)st.out[1],
                                              (int32_t *)st.out[2], cs()));
    return finish(st);
}
