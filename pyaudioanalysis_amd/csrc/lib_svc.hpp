// The multi-class probabilistic SVC of audioTrainTest.classifier_wrapper (audioTrainTest.py:84-93) for the shipped SVM models:
// an uploaded model behind a handle, host-buffer and device-buffer predict calls.  Kernels: kernels_svc.hpp (family_svc.hip).
#pragma once

struct PaaSvc {
    svc::SvcDev dev{};
    DevBlock block;               // every array of dev
};
static std::mutex g_svc_mu;

extern "C" int paa_svc_create(const double *support_vectors, int n_sv, int n_dims, const int32_t *n_support, int n_classes,
                              const double *dual_coef, const double *rho, const double *prob_a, const double *prob_b,
                              int kernel_type, double gamma, void **out_handle) {
    if (!out_handle) return fail(PAA_ERR_ARG, "null handle pointer");
    *out_handle = nullptr;
    if (!support_vectors || !n_support || !dual_coef || !rho || !prob_a || !prob_b) return fail(PAA_ERR_ARG, "null argument");
    if (n_classes < 2 || n_classes > svc::kMaxClasses) return fail(PAA_ERR_ARG, "%d classes: 2..%d are supported", n_classes, svc::kMaxClasses);
    if (n_dims < 1 || n_dims > svc::kMaxDims) return fail(PAA_ERR_ARG, "%d feature dimensions: 1..%d are supported", n_dims, svc::kMaxDims);
    if (kernel_type != 0 && kernel_type != 2) return fail(PAA_ERR_ARG, "kernel type %d: only LINEAR (0) and RBF (2)", kernel_type);
    if (n_sv < 1) return fail(PAA_ERR_ARG, "no support vectors");
    if (kernel_type == 2 && !(gamma > 0)) return fail(PAA_ERR_ARG, "RBF kernel needs gamma > 0");
    std::vector<int> ends(n_classes);
    long long total = 0;
    for (int c = 0; c < n_classes; ++c) {
        if (n_support[c] < 0) return fail(PAA_ERR_ARG, "negative n_support");
        total += n_support[c];
        ends[c] = (int)total;
    }
    if (total != n_sv) return fail(PAA_ERR_ARG, "n_support sums to %lld, not n_sv = %d", total, n_sv);
    int rc = ensure_init();
    if (rc) return rc;
    const int k = n_classes, pairs = k * (k - 1) / 2;
    const size_t n_sv_d = (size_t)n_sv * n_dims, n_coef = (size_t)(k - 1) * n_sv;
    std::unique_ptr<PaaSvc> h(new PaaSvc());
    BlockPart parts[] = {{support_vectors, n_sv_d * 8, 8}, {dual_coef, n_coef * 8, 8}, {rho, (size_t)pairs * 8, 8},
                         {prob_a, (size_t)pairs * 8, 8}, {prob_b, (size_t)pairs * 8, 8}, {ends.data(), (size_t)k * sizeof(int), 4}};
    if ((rc = block_upload(h->block, parts, 6, "the SVC model"))) return rc;
    h->dev.sv = (const double *)parts[0].dev;
    h->dev.coef = (const double *)parts[1].dev;
    h->dev.rho = (const double *)parts[2].dev;
    h->dev.prob_a = (const double *)parts[3].dev;
    h->dev.prob_b = (const double *)parts[4].dev;
    h->dev.class_end = (const int *)parts[5].dev;
    h->dev.n_sv = n_sv;
    h->dev.n_dims = n_dims;
    h->dev.k = k;
    h->dev.rbf = kernel_type == 2;
    h->dev.gamma = gamma;
    *out_handle = h.release();
    return PAA_OK;
}

extern "C" int paa_svc_destroy(void *handle) { return model_destroy((PaaSvc *)handle); }

extern "C" int paa_svc_num_classes(const void *handle) {
    return handle ? ((const PaaSvc *)handle)->dev.k : fail(PAA_ERR_ARG, "null handle");
}

constexpr int64_t kSvcMaxVec = 0x7fffffffLL * 16;      // grid limit of both kernels

extern "C" int paa_svc_dev_predict_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                                       const double *d_mean, const double *d_std, int32_t *d_label_index, double *d_proba) {
    int rc = model_check<PaaSvc>(handle, n_dims, ld, n_vec, kSvcMaxVec);
    if (rc) return rc;
    if (!d_feats || !d_mean || !d_std || !d_label_index || !d_proba) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    const svc::SvcDev &m = ((const PaaSvc *)handle)->dev;
    std::lock_guard<std::mutex> lk(g_svc_mu);
    {
        std::lock_guard<std::mutex> lk2(g_mu);
        if ((rc = scratch_reserve(g_svc_sums, (size_t)n_vec * m.k * (m.k - 1) * 8))) return rc;
    }
    LAUNCH_TRY("SVC", launch::svc(m, d_feats, (long long)ld, (long long)n_vec, d_mean, d_std, (double *)g_svc_sums.p, d_label_index,
                                  d_proba, cs()));
    return PAA_OK;
}

extern "C" int paa_svc_predict_f64(const void *handle, const double *feats, int n_dims, int64_t ld, int64_t n_vec,
                                   const double *mean, const double *std, int32_t *label_index, double *proba) {
    int rc = model_check<PaaSvc>(handle, n_dims, ld, n_vec, kSvcMaxVec);
    if (rc) return rc;
    if (!feats || !mean || !std || !label_index || !proba) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    const svc::SvcDev &m = ((const PaaSvc *)handle)->dev;
    Staged st;
    if ((rc = stage(st, feats, n_dims, ld, mean, std, (size_t)n_vec * m.k * (m.k - 1) * 8,
                    {{label_index, (size_t)n_vec * 4}, {proba, (size_t)n_vec * m.k * 8}})))
        return rc;
    LAUNCH_TRY("SVC", launch::svc(m, st.feats, (long long)ld, (long long)n_vec, st.mean, st.std, (double *)st.mid, (int32_t *)st.out[0],
                                  (double *)st.out[1], cs()));
    return finish(st);
}
