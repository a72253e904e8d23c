// Speaker diarization (audioSegmentation.speaker_diarization, :815-1056): the device-buffer entry points between the mid-term
// matrix and the HMM smoothing -- standardisation, the feature-row distances of the "outlier" filter and of the silhouette's
// a terms, k-means for every k of a sweep, k-means++ seeding's distance work, and the cluster-pair distance sums of the
// silhouette's b terms.  Kernels: kernels_diar.hpp (family_diar.hip).  Every call is synchronous on cs().
#pragma once

static GlobalScratch g_diar;          // work space of the call in flight
static std::mutex g_diar_mu;

static int diar_check(int n_dims, int64_t ld, int64_t n_vec) {
    if (n_dims < 1 || n_dims > hmm::kMaxDims) return fail(PAA_ERR_ARG, "%d feature dimensions: 1..%d are supported", n_dims, hmm::kMaxDims);
    return check_matrix(ld, n_vec, 0x7fffffffLL / 64);
}

// ks [nk] in 1..32, none above n_vec; returns the largest through kmax
static int diar_check_ks(const int32_t *ks, int nk, int64_t n_vec, int *kmax) {
    if (!ks || nk < 1 || nk > hmm::kMaxStates) return fail(PAA_ERR_ARG, "a sweep has 1..%d cluster counts", hmm::kMaxStates);
    *kmax = 0;
    for (int i = 0; i < nk; ++i) {
        if (ks[i] < 1 || ks[i] > hmm::kMaxStates) return fail(PAA_ERR_ARG, "%d clusters: 1..%d are supported", ks[i], hmm::kMaxStates);
        if (ks[i] > n_vec) return fail(PAA_ERR_ARG, "%d clusters for %lld vectors", ks[i], (long long)n_vec);
        *kmax = std::max(*kmax, (int)ks[i]);
    }
    return PAA_OK;
}

extern "C" int paa_diar_dev_standardize_f64(const double *d_feats, int n_dims, int64_t ld, int64_t n_vec, double *d_z, double *stats) {
    int rc = diar_check(n_dims, ld, n_vec);
    if (rc) return rc;
    if (!d_feats || !d_z || !stats) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    std::lock_guard<std::mutex> lk(g_diar_mu);
    if ((rc = scratch_reserve(g_diar, (size_t)3 * n_dims * 8))) return rc;
    LAUNCH_TRY("standardisation", launch::diar_standardize(d_feats, ld, n_vec, n_dims, d_z, ld, (double *)g_diar.p, cs()));
    HIP_TRY(hipMemcpyAsync(stats, g_diar.p, (size_t)3 * n_dims * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}

extern "C" int paa_diar_dev_select_rows_f64(const double *d_z, int n_dims, int64_t ld, int64_t n_vec, const int32_t *rows, int n_rows,
                                            double *d_out) {
    int rc = diar_check(n_dims, ld, n_vec);
    if (rc) return rc;
    if (!d_z || !rows || !d_out) return fail(PAA_ERR_ARG, "null buffer");
    if (n_rows < 1 || n_rows > n_dims) return fail(PAA_ERR_ARG, "%d rows of %d", n_rows, n_dims);
    for (int i = 0; i < n_rows; ++i)
        if (rows[i] < 0 || rows[i] >= n_dims) return fail(PAA_ERR_ARG, "row %d is outside 0..%d", rows[i], n_dims - 1);
    if ((rc = ensure_init())) return rc;
    std::lock_guard<std::mutex> lk(g_diar_mu);
    if ((rc = scratch_reserve(g_diar, (size_t)n_rows * 4))) return rc;
    HIP_TRY(hipMemcpyAsync(g_diar.p, rows, (size_t)n_rows * 4, hipMemcpyHostToDevice, cs()));
    LAUNCH_TRY("row selection", launch::diar_select_rows(d_z, ld, n_vec, (const int *)g_diar.p, n_rows, d_out, n_vec, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}

extern "C" int paa_diar_dev_dim_distances_f64(const double *d_z, int n_dims, int64_t ld, int64_t n_vec, const int32_t *d_labels,
                                              const int32_t *ks, int nk, double *colsum, double *pair_mean) {
    int rc = diar_check(n_dims, ld, n_vec);
    if (rc) return rc;
    if (!d_z || !colsum || !pair_mean) return fail(PAA_ERR_ARG, "null buffer");
    int kmax = 1;
    if (d_labels) {
        if ((rc = diar_check_ks(ks, nk, n_vec, &kmax))) return rc;
    } else {
        nk = 1;
    }
    if ((rc = ensure_init())) return rc;
    std::lock_guard<std::mutex> lk(g_diar_mu);
    const size_t slots = (size_t)nk * kmax, b_ks = up256((size_t)nk * 4), b_dist = up256(slots * n_dims * n_dims * 8),
                 b_col = up256(slots * n_dims * 8), b_pm = up256(slots * 8);
    if ((rc = scratch_reserve(g_diar, b_ks + b_dist + b_col + b_pm))) return rc;
    char *p = (char *)g_diar.p;
    int *d_ks = (int *)p;
    double *d_dist = (double *)(p + b_ks), *d_col = (double *)(p + b_ks + b_dist), *d_pm = (double *)(p + b_ks + b_dist + b_col);
    if (d_labels) HIP_TRY(hipMemcpyAsync(d_ks, ks, (size_t)nk * 4, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemsetAsync(d_col, 0, b_col + b_pm, cs()));
    LAUNCH_TRY("feature-row distance",
               launch::diar_dim_distances(d_z, ld, n_vec, n_dims, d_labels, d_ks, nk, kmax, d_dist, d_col, d_pm, cs()));
    HIP_TRY(hipMemcpyAsync(colsum, d_col, slots * n_dims * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(pair_mean, d_pm, slots * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}

static int diar_check_idx(const int64_t *idx, int n_pts, int64_t n_vec) {
    if (!idx || n_pts < 1) return fail(PAA_ERR_ARG, "no window indices");
    for (int i = 0; i < n_pts; ++i)
        if (idx[i] < 0 || idx[i] >= n_vec) return fail(PAA_ERR_ARG, "window %lld is outside 0..%lld", (long long)idx[i], (long long)n_vec - 1);
    return PAA_OK;
}

extern "C" int paa_diar_dev_sqdist_points_f64(const double *d_z, int n_dims, int64_t ld, int64_t n_vec, const int64_t *idx, int n_pts,
                                              double *out) {
    int rc = diar_check(n_dims, ld, n_vec);
    if (rc) return rc;
    if ((rc = diar_check_idx(idx, n_pts, n_vec))) return rc;
    if (n_pts > diar::kMaxPoints) return fail(PAA_ERR_ARG, "%d points: at most %d per call", n_pts, diar::kMaxPoints);
    if (!d_z || !out) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    std::lock_guard<std::mutex> lk(g_diar_mu);
    const size_t b_idx = up256((size_t)n_pts * 8), b_out = (size_t)n_pts * n_vec * 8;
    if ((rc = scratch_reserve(g_diar, b_idx + b_out))) return rc;
    long long *d_idx = (long long *)g_diar.p;
    double *d_out = (double *)((char *)g_diar.p + b_idx);
    HIP_TRY(hipMemcpyAsync(d_idx, idx, (size_t)n_pts * 8, hipMemcpyHostToDevice, cs()));
    LAUNCH_TRY("seeding distance", launch::diar_sqdist_points(d_z, ld, n_vec, n_dims, d_idx, n_pts, d_out, cs()));
    HIP_TRY(hipMemcpyAsync(out, d_out, b_out, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}

extern "C" int paa_diar_dev_get_points_f64(const double *d_z, int n_dims, int64_t ld, int64_t n_vec, const int64_t *idx, int n_pts,
                                           double *out) {
    int rc = diar_check(n_dims, ld, n_vec);
    if (rc) return rc;
    if ((rc = diar_check_idx(idx, n_pts, n_vec))) return rc;
    if (n_pts > 4096) return fail(PAA_ERR_ARG, "%d points: at most 4096 per call", n_pts);
    if (!d_z || !out) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    std::lock_guard<std::mutex> lk(g_diar_mu);
    const size_t b_idx = up256((size_t)n_pts * 8), b_out = (size_t)n_pts * n_dims * 8;
    if ((rc = scratch_reserve(g_diar, b_idx + b_out))) return rc;
    long long *d_idx = (long long *)g_diar.p;
    double *d_out = (double *)((char *)g_diar.p + b_idx);
    HIP_TRY(hipMemcpyAsync(d_idx, idx, (size_t)n_pts * 8, hipMemcpyHostToDevice, cs()));
    LAUNCH_TRY("point gather", launch::diar_get_points(d_z, ld, n_dims, d_idx, n_pts, d_out, cs()));
    HIP_TRY(hipMemcpyAsync(out, d_out, b_out, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}

extern "C" int paa_diar_dev_kmeans_f64(const double *d_z, int n_dims, int64_t ld, int64_t n_vec, const int32_t *ks, int nk,
                                       double *centers, double tol, int max_iter, int32_t *d_labels, int32_t *n_iter,
                                       double *inertia) {
    int rc = diar_check(n_dims, ld, n_vec);
    if (rc) return rc;
    int kmax = 0;
    if ((rc = diar_check_ks(ks, nk, n_vec, &kmax))) return rc;
    if (!d_z || !centers || !d_labels || !n_iter || !inertia) return fail(PAA_ERR_ARG, "null buffer");
    if (max_iter < 1 || !(tol >= 0.0)) return fail(PAA_ERR_ARG, "max_iter %d, tol %g", max_iter, tol);
    const size_t cells = (size_t)nk * hmm::kMaxStates * n_dims;
    for (int i = 0; i < nk; ++i)
        for (size_t j = 0; j < (size_t)ks[i] * n_dims; ++j)
            if (!std::isfinite(centers[(size_t)i * hmm::kMaxStates * n_dims + j])) return fail(PAA_ERR_ARG, "an initial centre is not finite");
    if ((rc = ensure_init())) return rc;
    std::lock_guard<std::mutex> lk(g_diar_mu);
    const size_t b_ks = up256((size_t)nk * 4), b_cen = up256(cells * 8), b_state = up256((size_t)nk * sizeof(diar::KmState)),
                 b_d2 = up256((size_t)nk * n_vec * 8), b_ints = up256((size_t)nk * diar::kIntsPerK * 4), b_in = up256((size_t)nk * 8);
    if ((rc = scratch_reserve(g_diar, b_ks + 2 * b_cen + b_state + b_d2 + b_ints + b_in))) return rc;
    char *p = (char *)g_diar.p;
    int *d_ks = (int *)p;                                   p += b_ks;
    double *d_cen = (double *)p;                            p += b_cen;
    double *d_sums = (double *)p;                           p += b_cen;
    diar::KmState *d_state = (diar::KmState *)p;            p += b_state;
    double *d_d2 = (double *)p;                             p += b_d2;
    int *d_ints = (int *)p;                                 p += b_ints;
    double *d_inertia = (double *)p;
    HIP_TRY(hipMemcpyAsync(d_ks, ks, (size_t)nk * 4, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemcpyAsync(d_cen, centers, cells * 8, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemsetAsync(d_sums, 0, cells * 8, cs()));
    HIP_TRY(hipMemsetAsync(d_state, 0, (size_t)nk * sizeof(diar::KmState), cs()));
    HIP_TRY(hipMemsetAsync(d_labels, 0xff, (size_t)nk * n_vec * 4, cs()));       // -1: no window keeps its label in iteration 1
    std::vector<diar::KmState> state(nk);
    for (int it = 0; it < max_iter; ++it) {
        LAUNCH_TRY("k-means", launch::diar_kmeans_step(d_z, ld, n_vec, n_dims, d_ks, nk, kmax, d_cen, d_state, d_labels, d_d2, d_ints,
                                                       d_sums, tol, max_iter, cs()));
        HIP_TRY(hipMemcpyAsync(state.data(), d_state, (size_t)nk * sizeof(diar::KmState), hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipStreamSynchronize(cs()));
        bool all = true;
        for (int i = 0; i < nk; ++i) all = all && state[i].done;
        if (all) break;
    }
    LAUNCH_TRY("k-means",
               launch::diar_kmeans_last(d_z, ld, n_vec, n_dims, d_ks, nk, kmax, d_cen, d_state, d_labels, d_d2, d_inertia, cs()));
    HIP_TRY(hipMemcpyAsync(centers, d_cen, cells * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(inertia, d_inertia, (size_t)nk * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    for (int i = 0; i < nk; ++i) n_iter[i] = state[i].n_iter;
    return PAA_OK;
}

extern "C" int paa_diar_dev_pair_sums_f64(const double *d_z, int n_dims, int64_t ld, int64_t n_vec, const int32_t *d_labels,
                                          const int32_t *ks, int nk, double *sums) {
    int rc = diar_check(n_dims, ld, n_vec);
    if (rc) return rc;
    int kmax = 0;
    if ((rc = diar_check_ks(ks, nk, n_vec, &kmax))) return rc;
    if (!d_z || !d_labels || !sums) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    std::vector<int> binoff(nk + 1, 0);
    for (int i = 0; i < nk; ++i) binoff[i + 1] = binoff[i] + ks[i] * ks[i];
    const int nbins = binoff[nk];
    const long long tiles = launch::diar_pair_tiles(n_vec), chunks = launch::diar_pair_chunks(n_vec);
    std::lock_guard<std::mutex> lk(g_diar_mu);
    const size_t b_ks = up256((size_t)nk * 4), b_off = up256((size_t)(nk + 1) * 4), b_part = up256((size_t)tiles * nbins * 8),
                 b_stage = up256((size_t)chunks * nbins * 8), b_S = up256((size_t)nbins * 8);
    if ((rc = scratch_reserve(g_diar, b_ks + b_off + b_part + b_stage + b_S))) return rc;
    char *p = (char *)g_diar.p;
    int *d_ks = (int *)p;                p += b_ks;
    int *d_off = (int *)p;               p += b_off;
    double *d_part = (double *)p;        p += b_part;
    double *d_stage = (double *)p;       p += b_stage;
    double *d_S = (double *)p;
    HIP_TRY(hipMemcpyAsync(d_ks, ks, (size_t)nk * 4, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemcpyAsync(d_off, binoff.data(), (size_t)(nk + 1) * 4, hipMemcpyHostToDevice, cs()));
    LAUNCH_TRY("cluster-pair",
               launch::diar_pair_sums(d_z, ld, n_vec, n_dims, d_labels, d_ks, nk, d_off, nbins, d_part, d_stage, d_S, cs()));
    std::vector<double> flat(nbins);
    HIP_TRY(hipMemcpyAsync(flat.data(), d_S, (size_t)nbins * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    const int W = hmm::kMaxStates;
    std::fill(sums, sums + (size_t)nk * W * W, 0.0);
    for (int i = 0; i < nk; ++i)
        for (int c = 0; c < ks[i]; ++c)
            for (int c2 = 0; c2 < ks[i]; ++c2) sums[((size_t)i * W + c) * W + c2] = flat[binoff[i] + c * ks[i] + c2];
    return PAA_OK;
}
