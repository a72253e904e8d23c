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
