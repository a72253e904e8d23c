// The multi-class probabilistic SVC of audioTrainTest.classifier_wrapper (audioTrainTest.py:84-93) for the shipped SVM models:
// an uploaded model behind a handle, host-buffer and device-buffer predict calls.  Kernels: kernels_svc.hpp (family_svc.hip).
#pragma once

struct PaaSvc {
    svc::SvcDev dev{};
    void *block = nullptr;        // one device allocation holding every array of dev
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
    const size_t doubles = n_sv_d + n_coef + 3 * (size_t)pairs;
    std::unique_ptr<PaaSvc> h(new PaaSvc());
    HIP_TRY(hipMalloc(&h->block, doubles * 8 + (size_t)k * sizeof(int)));
    double *d = (double *)h->block;
    h->dev.sv = d;
    h->dev.coef = d + n_sv_d;
    h->dev.rho = d + n_sv_d + n_coef;
    h->dev.prob_a = h->dev.rho + pairs;
    h->dev.prob_b = h->dev.prob_a + pairs;
    h->dev.class_end = (const int *)(d + doubles);
    h->dev.n_sv = n_sv;
    h->dev.n_dims = n_dims;
    h->dev.k = k;
    h->dev.rbf = kernel_type == 2;
    h->dev.gamma = gamma;
    auto fail_free = [&](int code) { (void)hipFree(h->block); return code; };
    if (hipMemcpy((void *)h->dev.sv, support_vectors, n_sv_d * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((void *)h->dev.coef, dual_coef, n_coef * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((void *)h->dev.rho, rho, (size_t)pairs * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((void *)h->dev.prob_a, prob_a, (size_t)pairs * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((void *)h->dev.prob_b, prob_b, (size_t)pairs * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((void *)h->dev.class_end, ends.data(), (size_t)k * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
        return fail_free(fail(PAA_ERR_HIP, "uploading the SVC model failed"));
    *out_handle = h.release();
    return PAA_OK;
}

extern "C" int paa_svc_destroy(void *handle) {
    if (!handle) return PAA_OK;
    PaaSvc *h = (PaaSvc *)handle;
    const hipError_t e = h->block ? hipFree(h->block) : hipSuccess;
    delete h;
    return e == hipSuccess ? PAA_OK : fail(PAA_ERR_HIP, "hipFree: %s", hipGetErrorString(e));
}

extern "C" int paa_svc_num_classes(const void *handle) {
    return handle ? ((const PaaSvc *)handle)->dev.k : fail(PAA_ERR_ARG, "null handle");
}

static int svc_check(const void *handle, int n_dims, int64_t ld, int64_t n_vec) {
    if (!handle) return fail(PAA_ERR_ARG, "null handle");
    const PaaSvc *h = (const PaaSvc *)handle;
    if (n_dims != h->dev.n_dims) return fail(PAA_ERR_ARG, "feature vectors have %d dims, the model %d", n_dims, h->dev.n_dims);
    if (n_vec < 1 || ld < n_vec) return fail(PAA_ERR_ARG, "bad feature matrix: %lld vectors, ld %lld", (long long)n_vec, (long long)ld);
    if (n_vec > 0x7fffffffLL * 16) return fail(PAA_ERR_ARG, "too many vectors");      // grid limit of both kernels
    return PAA_OK;
}

extern "C" int paa_svc_dev_predict_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                                       const double *d_mean, const double *d_std, int32_t *d_label_index, double *d_proba) {
    int rc = svc_check(handle, n_dims, ld, n_vec);
    if (rc) return rc;
    if (!d_feats || !d_mean || !d_std || !d_label_index || !d_proba) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    const svc::SvcDev &m = ((const PaaSvc *)handle)->dev;
    std::lock_guard<std::mutex> lk(g_svc_mu);
    {
        std::lock_guard<std::mutex> lk2(g_mu);
        if ((rc = scratch_reserve(g_svc_sums, (size_t)n_vec * m.k * (m.k - 1) * 8))) return rc;
    }
    if (launch::svc(m, d_feats, (long long)ld, (long long)n_vec, d_mean, d_std, (double *)g_svc_sums.p, d_label_index, d_proba,
                    cs()))
        return fail(PAA_ERR_HIP, "SVC launch failed: %s", hipGetErrorString(hipGetLastError()));
    return PAA_OK;
}

extern "C" int paa_svc_predict_f64(const void *handle, const double *feats, int n_dims, int64_t ld, int64_t n_vec,
                                   const double *mean, const double *std, int32_t *label_index, double *proba) {
    int rc = svc_check(handle, n_dims, ld, n_vec);
    if (rc) return rc;
    if (!feats || !mean || !std || !label_index || !proba) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    const svc::SvcDev &m = ((const PaaSvc *)handle)->dev;
    LaneGuard lane;       // own stream + scratch for this call (see Lane)
    const size_t fb = (size_t)n_dims * ld * 8, sums = (size_t)n_vec * m.k * (m.k - 1) * 8;
    const size_t lab = ((size_t)n_vec * 4 + 255) / 256 * 256, pb = (size_t)n_vec * m.k * 8;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if ((rc = scratch_reserve(lane.l->in, fb + (size_t)2 * n_dims * 8))) return rc;
        if ((rc = scratch_reserve(lane.l->mid, sums))) return rc;
        if ((rc = scratch_reserve(lane.l->out, lab + pb))) return rc;
    }
    double *d_feats = (double *)lane.l->in.p, *d_mean = d_feats + (size_t)n_dims * ld, *d_std = d_mean + n_dims;
    int32_t *d_label = (int32_t *)lane.l->out.p;
    double *d_proba = (double *)((char *)lane.l->out.p + lab);
    HIP_TRY(hipMemcpyAsync(d_feats, feats, fb, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemcpyAsync(d_mean, mean, (size_t)n_dims * 8, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemcpyAsync(d_std, std, (size_t)n_dims * 8, hipMemcpyHostToDevice, cs()));
    if (launch::svc(m, d_feats, (long long)ld, (long long)n_vec, d_mean, d_std, (double *)lane.l->mid.p, d_label, d_proba, cs()))
        return fail(PAA_ERR_HIP, "SVC launch failed: %s", hipGetErrorString(hipGetLastError()));
    HIP_TRY(hipMemcpyAsync(label_index, d_label, (size_t)n_vec * 4, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(proba, d_proba, pb, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}
