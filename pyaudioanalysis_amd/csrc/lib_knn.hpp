// The k-nearest-neighbour classifier of audioTrainTest.Knn (audioTrainTest.py:33-49) for the shipped knn_* models: an
// uploaded model behind a handle, host-buffer and device-buffer predict calls.  Kernel: kernels_knn.hpp (family_knn.hip).
#pragma once

struct PaaKnn {
    knn::KnnDev dev{};
    void *block = nullptr;        // one device allocation: training rows, then labels
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
    const size_t n_td = (size_t)n_train * n_dims;
    std::unique_ptr<PaaKnn> h(new PaaKnn());
    HIP_TRY(hipMalloc(&h->block, n_td * 8 + (size_t)n_train * sizeof(int)));
    h->dev.train = (const double *)h->block;
    h->dev.labels = (const int *)((const double *)h->block + n_td);
    h->dev.n_train = n_train;
    h->dev.n_dims = n_dims;
    h->dev.n_classes = n_classes;
    h->dev.k = k;
    if (hipMemcpy((void *)h->dev.train, train, n_td * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((void *)h->dev.labels, labels, (size_t)n_train * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(h->block);
        return fail(PAA_ERR_HIP, "uploading the kNN model failed");
    }
    *out_handle = h.release();
    return PAA_OK;
}

extern "C" int paa_knn_destroy(void *handle) {
    if (!handle) return PAA_OK;
    PaaKnn *h = (PaaKnn *)handle;
    const hipError_t e = h->block ? hipFree(h->block) : hipSuccess;
    delete h;
    return e == hipSuccess ? PAA_OK : fail(PAA_ERR_HIP, "hipFree: %s", hipGetErrorString(e));
}

extern "C" int paa_knn_num_classes(const void *handle) {
    return handle ? ((const PaaKnn *)handle)->dev.n_classes : fail(PAA_ERR_ARG, "null handle");
}

static int knn_check(const void *handle, int n_dims, int64_t ld, int64_t n_vec) {
    if (!handle) return fail(PAA_ERR_ARG, "null handle");
    const PaaKnn *h = (const PaaKnn *)handle;
    if (n_dims != h->dev.n_dims) return fail(PAA_ERR_ARG, "feature vectors have %d dims, the model %d", n_dims, h->dev.n_dims);
    if (n_vec < 1 || ld < n_vec) return fail(PAA_ERR_ARG, "bad feature matrix: %lld vectors, ld %lld", (long long)n_vec, (long long)ld);
    if (n_vec > 0x7fffffffLL * knn::kQueriesPerBlock) return fail(PAA_ERR_ARG, "too many vectors");    // grid limit
    return PAA_OK;
}

extern "C" int paa_knn_dev_predict_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                                       const double *d_mean, const double *d_std, int32_t *d_label_index, double *d_proba,
                                       int32_t *d_neighbors) {
    int rc = knn_check(handle, n_dims, ld, n_vec);
    if (rc) return rc;
    if (!d_feats || !d_mean || !d_std || !d_label_index || !d_proba) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    if (launch::knn(((const PaaKnn *)handle)->dev, d_feats, (long long)ld, (long long)n_vec, d_mean, d_std, d_label_index,
                    d_proba, d_neighbors, cs()))
        return fail(PAA_ERR_HIP, "kNN launch failed: %s", hipGetErrorString(hipGetLastError()));
    return PAA_OK;
}

extern "C" int paa_knn_predict_f64(const void *handle, const double *feats, int n_dims, int64_t ld, int64_t n_vec,
                                   const double *mean, const double *std, int32_t *label_index, double *proba,
                                   int32_t *neighbors) {
    int rc = knn_check(handle, n_dims, ld, n_vec);
    if (rc) return rc;
    if (!feats || !mean || !std || !label_index || !proba) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    const knn::KnnDev &m = ((const PaaKnn *)handle)->dev;
    LaneGuard lane;       // own stream + scratch for this call (see Lane)
    const size_t fb = (size_t)n_dims * ld * 8;
    const size_t lab = ((size_t)n_vec * 4 + 255) / 256 * 256, pb = ((size_t)n_vec * m.n_classes * 8 + 255) / 256 * 256;
    const size_t nbb = neighbors ? (size_t)n_vec * m.k * 4 : 0;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if ((rc = scratch_reserve(lane.l->in, fb + (size_t)2 * n_dims * 8))) return rc;
        if ((rc = scratch_reserve(lane.l->out, lab + pb + nbb))) return rc;
    }
    double *d_feats = (double *)lane.l->in.p, *d_mean = d_feats + (size_t)n_dims * ld, *d_std = d_mean + n_dims;
    int32_t *d_label = (int32_t *)lane.l->out.p;
    double *d_proba = (double *)((char *)lane.l->out.p + lab);
    int32_t *d_nb = neighbors ? (int32_t *)((char *)lane.l->out.p + lab + pb) : nullptr;
    HIP_TRY(hipMemcpyAsync(d_feats, feats, fb, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemcpyAsync(d_mean, mean, (size_t)n_dims * 8, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemcpyAsync(d_std, std, (size_t)n_dims * 8, hipMemcpyHostToDevice, cs()));
    if (launch::knn(m, d_feats, (long long)ld, (long long)n_vec, d_mean, d_std, d_label, d_proba, d_nb, cs()))
        return fail(PAA_ERR_HIP, "kNN launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIP_TRY(hipMemcpyAsync(label_index, d_label, (size_t)n_vec * 4, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(proba, d_proba, (size_t)n_vec * m.n_classes * 8, hipMemcpyDeviceToHost, cs()));
    if (neighbors) HIP_TRY(hipMemcpyAsync(neighbors, d_nb, nbb, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}
