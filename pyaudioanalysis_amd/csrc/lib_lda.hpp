// The LDA step of speaker diarization (audioSegmentation.speaker_diarization, :880-934, lda_dim > 0): the device-buffer entry
// points of the O(n) parts of scikit-learn's svd-solver LinearDiscriminantAnalysis -- class means and pooled within-class
// deviations, the Gram matrix of the centred, scaled windows, and the projection.  The two small symmetric eigenproblems
// between them stay with the caller.  Kernels: kernels_lda.hpp (family_lda.hip).  Every call is synchronous on cs().
#pragma once

static GlobalScratch g_lda;           // work space of the call in flight
static std::mutex g_lda_mu;

static int lda_check(int n_dims, int64_t ld, int64_t n_vec) {
    if (n_dims < 1 || n_dims > hmm::kMaxDims) return fail(PAA_ERR_ARG, "%d feature dimensions: 1..%d are supported", n_dims, hmm::kMaxDims);
    return check_matrix(ld, n_vec, 0x7fffffffLL / 64);
}

// run_offsets [n_classes + 1]: 0 = off[0] < off[1] < ... < off[n_classes] = n_vec
static int lda_check_runs(const int64_t *off, int64_t n_classes, int64_t n_vec) {
    if (!off || n_classes < 1 || n_classes > n_vec) return fail(PAA_ERR_ARG, "%lld classes for %lld vectors", (long long)n_classes, (long long)n_vec);
    if (off[0] != 0 || off[n_classes] != n_vec) return fail(PAA_ERR_ARG, "the class runs must cover vectors 0..%lld", (long long)n_vec - 1);
    for (int64_t c = 0; c < n_classes; ++c)
        if (off[c + 1] <= off[c]) return fail(PAA_ERR_ARG, "class %lld has no vectors", (long long)c);
    return PAA_OK;
}

extern "C" int paa_lda_dev_class_stats_f64(const double *d_x, int n_dims, int64_t ld, int64_t n_vec, const int64_t *run_offsets,
                                           int64_t n_classes, double *means, double *within_std) {
    int rc = lda_check(n_dims, ld, n_vec);
    if (rc) return rc;
    if ((rc = lda_check_runs(run_offsets, n_classes, n_vec))) return rc;
    if (!d_x || !means || !within_std) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    std::lock_guard<std::mutex> lk(g_lda_mu);
    const size_t b_off = up256((size_t)(n_classes + 1) * 8), b_cd = up256((size_t)n_classes * n_dims * 8), b_std = up256((size_t)n_dims * 8);
    if ((rc = scratch_reserve(g_lda, b_off + 3 * b_cd + b_std))) return rc;
    char *p = (char *)g_lda.p;
    long long *d_off = (long long *)p;      p += b_off;
    double *d_means = (double *)p;          p += b_cd;
    double *d_dev = (double *)p;            p += b_cd;
    double *d_sq = (double *)p;             p += b_cd;
    double *d_std = (double *)p;
    HIP_TRY(hipMemcpyAsync(d_off, run_offsets, (size_t)(n_classes + 1) * 8, hipMemcpyHostToDevice, cs()));
    LAUNCH_TRY("class statistics", launch::lda_class_stats(d_x, ld, n_vec, n_dims, d_off, n_classes, d_means, d_dev, d_sq, d_std, cs()));
    HIP_TRY(hipMemcpyAsync(means, d_means, (size_t)n_classes * n_dims * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(within_std, d_std, (size_t)n_dims * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}

extern "C" int paa_lda_dev_within_gram_f64(const double *d_x, int n_dims, int64_t ld, int64_t n_vec, const int64_t *run_offsets,
                                           int64_t n_classes, const double *means, const double *within_std, double fac,
                                           double *gram) {
    int rc = lda_check(n_dims, ld, n_vec);
    if (rc) return rc;
    if ((rc = lda_check_runs(run_offsets, n_classes, n_vec))) return rc;
    if (!d_x || !means || !within_std || !gram) return fail(PAA_ERR_ARG, "null buffer");
    if (!(fac > 0.0) || !std::isfinite(fac)) return fail(PAA_ERR_ARG, "fac %g", fac);
    std::vector<double> rscale(n_dims);
    for (int d = 0; d < n_dims; ++d) {
        if (!(within_std[d] > 0.0) || !std::isfinite(within_std[d])) return fail(PAA_ERR_ARG, "within-class deviation %g of dimension %d", within_std[d], d);
        rscale[d] = std::sqrt(fac) / within_std[d];
    }
    if ((rc = ensure_init())) return rc;
    std::lock_guard<std::mutex> lk(g_lda_mu);
    const long long chunks = launch::lda_gram_chunks(n_vec);
    const size_t b_off = up256((size_t)(n_classes + 1) * 8), b_cd = up256((size_t)n_classes * n_dims * 8), b_rs = up256((size_t)n_dims * 8),
                 b_cls = up256((size_t)n_vec * 4), b_g = up256((size_t)n_dims * n_dims * 8), b_part = up256((size_t)chunks * n_dims * n_dims * 8);
    if ((rc = scratch_reserve(g_lda, b_off + b_cd + b_rs + b_cls + b_g + b_part))) return rc;
    char *p = (char *)g_lda.p;
    long long *d_off = (long long *)p;      p += b_off;
    double *d_means = (double *)p;          p += b_cd;
    double *d_rs = (double *)p;             p += b_rs;
    int *d_cls = (int *)p;                  p += b_cls;
    double *d_G = (double *)p;              p += b_g;
    double *d_part = (double *)p;
    HIP_TRY(hipMemcpyAsync(d_off, run_offsets, (size_t)(n_classes + 1) * 8, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemcpyAsync(d_means, means, (size_t)n_classes * n_dims * 8, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemcpy(d_rs, rscale.data(), (size_t)n_dims * 8, hipMemcpyHostToDevice));      // synchronous: rscale is a local
    LAUNCH_TRY("within-class Gram", launch::lda_within_gram(d_x, ld, n_vec, n_dims, d_off, n_classes, d_means, d_rs, d_cls, d_part, d_G, cs()));
    HIP_TRY(hipMemcpyAsync(gram, d_G, (size_t)n_dims * n_dims * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}

extern "C" int paa_lda_dev_project_f64(const double *d_x, int n_dims, int64_t ld, int64_t n_vec, const double *xbar,
                                       const double *scalings, int n_out, double *d_y, int64_t ld_y) {
    int rc = lda_check(n_dims, ld, n_vec);
    if (rc) return rc;
    if (n_out < 1 || n_out > n_dims) return fail(PAA_ERR_ARG, "%d output dimensions of %d", n_out, n_dims);
    if (ld_y < n_vec) return fail(PAA_ERR_ARG, "bad output matrix: %lld vectors, ld %lld", (long long)n_vec, (long long)ld_y);
    if (!d_x || !xbar || !scalings || !d_y) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    std::lock_guard<std::mutex> lk(g_lda_mu);
    const size_t b_xbar = up256((size_t)n_dims * 8), b_s = (size_t)n_dims * n_out * 8;
    if ((rc = scratch_reserve(g_lda, b_xbar + b_s))) return rc;
    double *d_xbar = (double *)g_lda.p, *d_s = (double *)((char *)g_lda.p + b_xbar);
    HIP_TRY(hipMemcpyAsync(d_xbar, xbar, (size_t)n_dims * 8, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemcpyAsync(d_s, scalings, b_s, hipMemcpyHostToDevice, cs()));
    LAUNCH_TRY("projection", launch::lda_project(d_x, ld, n_vec, n_dims, d_xbar, d_s, n_out, d_y, ld_y, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}
