// The regression models of audioTrainTest.regression_wrapper (audioTrainTest.py:96-111) for the "svm" / "svm_rbf" types --
// scikit-learn's epsilon-SVR as file_regression (:1099-1151) and evaluate_regression (:774-855) apply it: a BANK of models
// that share n_dims, each with its own standardisation, uploaded once behind a handle; host-buffer and device-buffer
// predict calls.  Kernel: kernels_svr.hpp (family_svr.hip).
#pragma once

struct PaaSvr {
    svr::SvrDev dev{};
    DevBlock block;               // every array of dev
};

extern "C" int paa_svr_create(int n_models, const int64_t *sv_offsets, const double *support_vectors, const double *dual_coef,
                              const double *rho, const int32_t *kernel_type, const double *gamma, const double *mean,
                              const double *std, int n_dims, void **out_handle) {
    if (!out_handle) return fail(PAA_ERR_ARG, "null handle pointer");
    *out_handle = nullptr;
    if (!sv_offsets || !rho || !kernel_type || !gamma || !mean || !std) return fail(PAA_ERR_ARG, "null argument");
    if (n_models < 1 || n_models > svr::kMaxModels) return fail(PAA_ERR_ARG, "%d models: 1..%d are supported", n_models, svr::kMaxModels);
    if (n_dims < 1 || n_dims > svr::kMaxDims) return fail(PAA_ERR_ARG, "%d feature dimensions: 1..%d are supported", n_dims, svr::kMaxDims);
    if (sv_offsets[0] != 0) return fail(PAA_ERR_ARG, "support-vector offsets must start at 0");
    for (int m = 0; m < n_models; ++m) {
        if (sv_offsets[m + 1] < sv_offsets[m]) return fail(PAA_ERR_ARG, "support-vector offsets decrease at model %d", m);
        if (kernel_type[m] != 0 && kernel_type[m] != 2)
            return fail(PAA_ERR_ARG, "model %d: kernel type %d: only LINEAR (0) and RBF (2)", m, kernel_type[m]);
        if (kernel_type[m] == 2 && !(gamma[m] > 0)) return fail(PAA_ERR_ARG, "model %d: RBF kernel needs gamma > 0", m);
    }
    const int64_t total = sv_offsets[n_models];
    if (total > 0 && (!support_vectors || !dual_coef)) return fail(PAA_ERR_ARG, "null argument");
    int rc = ensure_init();
    if (rc) return rc;
    const size_t row = (size_t)n_dims * 8;
    std::vector<int> rbf(n_models), same(n_models, 0);
    for (int m = 0; m < n_models; ++m) {
        rbf[m] = kernel_type[m] == 2;
        if (m > 0)
            same[m] = !memcmp(mean + (size_t)m * n_dims, mean + (size_t)(m - 1) * n_dims, row) &&
                      !memcmp(std + (size_t)m * n_dims, std + (size_t)(m - 1) * n_dims, row);
    }
    static const double none = 0.0;          // a bank without any support vector still uploads one (unread) element
    std::unique_ptr<PaaSvr> h(new PaaSvr());
    BlockPart parts[] = {{total ? support_vectors : &none, total ? (size_t)total * row : 8, 8},
                         {total ? dual_coef : &none, total ? (size_t)total * 8 : 8, 8},
                         {sv_offsets, (size_t)(n_models + 1) * 8, 8},
                         {rho, (size_t)n_models * 8, 8},
                         {gamma, (size_t)n_models * 8, 8},
                         {mean, (size_t)n_models * row, 8},
                         {std, (size_t)n_models * row, 8},
                         {rbf.data(), (size_t)n_models * sizeof(int), 4},
                         {same.data(), (size_t)n_models * sizeof(int), 4}};
    if ((rc = block_upload(h->block, parts, 9, "the SVR bank"))) return rc;
    h->dev.sv = (const double *)parts[0].dev;
    h->dev.coef = (const double *)parts[1].dev;
    h->dev.sv_off = (const long long *)parts[2].dev;
    h->dev.rho = (const double *)parts[3].dev;
    h->dev.gamma = (const double *)parts[4].dev;
    h->dev.mean = (const double *)parts[5].dev;
    h->dev.scale = (const double *)parts[6].dev;
    h->dev.rbf = (const int *)parts[7].dev;
    h->dev.same_prev = (const int *)parts[8].dev;
    h->dev.n_models = n_models;
    h->dev.n_dims = n_dims;
    *out_handle = h.release();
    return PAA_OK;
}

extern "C" int paa_svr_destroy(void *handle) { return model_destroy((PaaSvr *)handle); }

extern "C" int paa_svr_num_models(const void *handle) {
    return handle ? ((const PaaSvr *)handle)->dev.n_models : fail(PAA_ERR_ARG, "null handle");
}

// windows per workgroup, models per workgroup, support vectors per LDS tile, lanes per window group (for the edge tests)
extern "C" int paa_debug_svr_geometry(int32_t *out4) {
    if (!out4) return fail(PAA_ERR_ARG, "null");
    launch::svr_geometry(out4);
    return PAA_OK;
}

constexpr int64_t kSvrMaxVec = 0x7fffffffLL * 16;      // grid limit

extern "C" int paa_svr_dev_predict_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                                       double *d_out, int64_t ld_out) {
    int rc = model_check<PaaSvr>(handle, n_dims, ld, n_vec, kSvrMaxVec);
    if (rc) return rc;
    if (ld_out < n_vec) return fail(PAA_ERR_ARG, "output rows of %lld for %lld vectors", (long long)ld_out, (long long)n_vec);
    if (!d_feats || !d_out) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    LAUNCH_TRY("SVR", launch::svr(((const PaaSvr *)handle)->dev, d_feats, (long long)ld, (long long)n_vec, d_out, (long long)ld_out, cs()));
    return PAA_OK;
}

extern "C" int paa_svr_predict_f64(const void *handle, const double *feats, int n_dims, int64_t ld, int64_t n_vec, double *out) {
    int rc = model_check<PaaSvr>(handle, n_dims, ld, n_vec, kSvrMaxVec);
    if (rc) return rc;
    if (!feats || !out) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    const svr::SvrDev &m = ((const PaaSvr *)handle)->dev;
    Staged st;
    if ((rc = stage(st, feats, n_dims, ld, nullptr, nullptr, 0, {{out, (size_t)m.n_models * n_vec * 8}}))) return rc;
    LAUNCH_TRY("SVR", launch::svr(m, st.feats, (long long)ld, (long long)n_vec, (double *)st.out[0], (long long)n_vec, cs()));
    return finish(st);
}
