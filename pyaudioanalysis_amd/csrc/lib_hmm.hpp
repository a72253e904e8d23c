// Gaussian HMM segmentation (audioSegmentation.hmm_segmentation / train_hmm_compute_statistics, :287-492): an uploaded model
// behind a handle, host-buffer and device-buffer decode calls, the emission matrix on its own, and the training
// statistics.  Kernels: kernels_hmm.hpp (family_hmm.hip).
#pragma once

struct PaaHmm {
    hmm::HmmDev dev{};
    DevBlock block;                   // the model tables
    Scratch work;                     // emission matrix, back-pointers, segment tables, block products: grown on demand
    std::vector<hmm::Segment> segs;   // host copies of the last call's tables: their upload is asynchronous
    std::vector<long long> seq_seg;
    std::mutex mu;
};
static GlobalScratch g_hmm_stats;     // labels, counts, means, deviations of the training-statistics entry points
static std::mutex g_hmm_stats_mu;

static bool hmm_is_distribution(const double *p, int n) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
        if (!(p[i] >= 0.0) || !std::isfinite(p[i])) return false;
        s += p[i];
    }
    return std::fabs(s - 1.0) <= 1e-8;
}

extern "C" int paa_hmm_create(const double *startprob, const double *transmat, const double *means, const double *covars,
                              int n_states, int n_dims, void **out_handle) {
    if (!out_handle) return fail(PAA_ERR_ARG, "null handle pointer");
    *out_handle = nullptr;
    if (!startprob || !transmat || !means || !covars) return fail(PAA_ERR_ARG, "null argument");
    if (n_states < 1 || n_states > hmm::kMaxStates) return fail(PAA_ERR_ARG, "%d states: 1..%d are supported", n_states, hmm::kMaxStates);
    if (n_dims < 1 || n_dims > hmm::kMaxDims) return fail(PAA_ERR_ARG, "%d feature dimensions: 1..%d are supported", n_dims, hmm::kMaxDims);
    const int K = n_states, D = n_dims;
    for (int i = 0; i < K * D; ++i) {
        if (!std::isfinite(means[i])) return fail(PAA_ERR_ARG, "means[%d][%d] is not finite", i / D, i % D);
        if (!std::isfinite(covars[i]) || !(covars[i] > 0.0))
            return fail(PAA_ERR_ARG, "covars[%d][%d] = %g: must be finite and positive", i / D, i % D, covars[i]);
    }
    if (!hmm_is_distribution(startprob, K)) return fail(PAA_ERR_ARG, "startprob must be non-negative and sum to 1");
    for (int i = 0; i < K; ++i)
        if (!hmm_is_distribution(transmat + (size_t)i * K, K))
            return fail(PAA_ERR_ARG, "transmat row %d must be non-negative and sum to 1", i);
    int rc = ensure_init();
    if (rc) return rc;
    int kp = 2;
    while (kp < K) kp <<= 1;
    const double ninf = -std::numeric_limits<double>::infinity();
    std::vector<double> tab((size_t)2 * D * kp + 2 * kp + (size_t)kp * kp, 0.0);
    double *mu = tab.data(), *inv = mu + (size_t)D * kp, *cst = inv + (size_t)D * kp, *logpi = cst + kp, *logA = logpi + kp;
    for (int k = 0; k < kp; ++k) {
        logpi[k] = k < K ? std::log(startprob[k]) : ninf;          // log 0 = -inf
        for (int j = 0; j < kp; ++j) logA[k * kp + j] = (k < K && j < K) ? std::log(transmat[k * K + j]) : ninf;
        if (k >= K) continue;
        double sum_log = 0.0;
        for (int d = 0; d < D; ++d) {
            mu[d * kp + k] = means[k * D + d];
            inv[d * kp + k] = 1.0 / covars[k * D + d];
            sum_log += std::log(covars[k * D + d]);
        }
        cst[k] = D * std::log(2.0 * M_PI) + sum_log;
    }
    std::unique_ptr<PaaHmm> h(new PaaHmm());
    BlockPart part = {tab.data(), tab.size() * 8, 8};
    if ((rc = block_upload(h->block, &part, 1, "the HMM"))) return rc;
    const double *base = (const double *)part.dev;
    h->dev.mu = base;
    h->dev.inv = base + (size_t)D * kp;
    h->dev.cst = base + (size_t)2 * D * kp;
    h->dev.logpi = h->dev.cst + kp;
    h->dev.logA = h->dev.logpi + kp;
    h->dev.n_states = K;
    h->dev.n_dims = D;
    h->dev.kp = kp;
    *out_handle = h.release();
    return PAA_OK;
}

extern "C" int paa_hmm_destroy(void *handle) {
    return model_destroy((PaaHmm *)handle, handle ? ((PaaHmm *)handle)->work.p : nullptr);
}

extern "C" int paa_hmm_num_states(const void *handle) {
    return handle ? ((const PaaHmm *)handle)->dev.n_states : fail(PAA_ERR_ARG, "null handle");
}

constexpr int64_t kHmmMaxVec = 0x7fffffffLL;

static int hmm_check_offsets(const int64_t *offsets, int64_t n_seq, int64_t n_vec) {
    if (!offsets) return fail(PAA_ERR_ARG, "null offsets");
    if (n_seq < 1 || n_seq > n_vec) return fail(PAA_ERR_ARG, "%lld sequences over %lld vectors", (long long)n_seq, (long long)n_vec);
    if (offsets[0] != 0 || offsets[n_seq] != n_vec) return fail(PAA_ERR_ARG, "offsets must run from 0 to the number of vectors");
    for (int64_t q = 0; q < n_seq; ++q)
        if (offsets[q + 1] <= offsets[q]) return fail(PAA_ERR_ARG, "sequence %lld is empty", (long long)q);
    return PAA_OK;
}

// emission + Viterbi on cs(); block_rows <= 0: hmm::kBlockRows
static int hmm_decode_core(PaaHmm *h, const double *d_feats, int64_t ld, int64_t n_vec, const int64_t *offsets, int64_t n_seq,
                           int32_t *d_states, double *d_logprob, int64_t block_rows) {
    const hmm::HmmDev &m = h->dev;
    const long long L = block_rows > 0 ? block_rows : hmm::kBlockRows;
    std::lock_guard<std::mutex> lk(h->mu);
    h->segs.clear();
    h->seq_seg.assign(1, 0);
    int multi = 0;
    for (int64_t q = 0; q < n_seq; ++q) {
        for (long long r = offsets[q]; r < offsets[q + 1]; r += L) {
            const long long r1 = std::min<long long>(r + L, offsets[q + 1]);
            h->segs.push_back(hmm::Segment{r, r1, r == offsets[q], r1 == offsets[q + 1]});
        }
        const long long n = (long long)h->segs.size();
        if (n - h->seq_seg.back() > 1) multi = 1;
        h->seq_seg.push_back(n);
    }
    const size_t n_seg = h->segs.size(), kp = m.kp;
    if (n_seg * m.n_states > 0x7fffffffULL) return fail(PAA_ERR_ARG, "too many segments");
    const size_t b_B = up256((size_t)n_vec * m.n_states * 8), b_M = multi ? up256(n_seg * kp * kp * 8) : 0,
                 b_V = up256(n_seg * kp * 8), b_segs = up256(n_seg * sizeof(hmm::Segment)),
                 b_seq = up256((size_t)(n_seq + 1) * 8), b_end = up256(n_seg * 4), b_psi = up256((size_t)n_vec * kp),
                 b_map = up256(n_seg * kp);
    int rc = scratch_reserve(h->work, b_B + b_M + 2 * b_V + b_segs + b_seq + b_end + b_psi + b_map);
    if (rc) return rc;
    char *p = (char *)h->work.p;
    double *d_B = (double *)p;               p += b_B;
    double *d_M = (double *)p;               p += b_M;
    double *d_V = (double *)p;               p += b_V;
    double *d_Vout = (double *)p;            p += b_V;
    hmm::Segment *d_segs = (hmm::Segment *)p; p += b_segs;
    long long *d_seq = (long long *)p;       p += b_seq;
    int *d_end = (int *)p;                   p += b_end;
    unsigned char *d_psi = (unsigned char *)p; p += b_psi;
    unsigned char *d_map = (unsigned char *)p;
    HIP_TRY(hipMemcpyAsync(d_segs, h->segs.data(), n_seg * sizeof(hmm::Segment), hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemcpyAsync(d_seq, h->seq_seg.data(), (size_t)(n_seq + 1) * 8, hipMemcpyHostToDevice, cs()));
    LAUNCH_TRY("HMM emission", launch::hmm_emission(m, d_feats, (long long)ld, (long long)n_vec, d_B, cs()));
    LAUNCH_TRY("HMM decode", launch::hmm_decode(m, d_B, d_segs, (long long)n_seg, d_seq, (long long)n_seq, multi, d_M, d_V, d_Vout, d_psi,
                                                d_map, d_end, d_states, d_logprob, cs()));
    return PAA_OK;
}

static int hmm_dev_decode(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                          const int64_t *offsets, int64_t n_seq, int32_t *d_states, double *d_logprob, int64_t block_rows) {
    int rc = model_check<PaaHmm>(handle, n_dims, ld, n_vec, kHmmMaxVec);
    if (rc) return rc;
    if ((rc = hmm_check_offsets(offsets, n_seq, n_vec))) return rc;
    if (!d_feats || !d_states || !d_logprob) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    return hmm_decode_core((PaaHmm *)handle, d_feats, ld, n_vec, offsets, n_seq, d_states, d_logprob, block_rows);
}

extern "C" int paa_hmm_dev_decode_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                                      const int64_t *offsets, int64_t n_seq, int32_t *d_states, double *d_logprob) {
    return hmm_dev_decode(handle, d_feats, n_dims, ld, n_vec, offsets, n_seq, d_states, d_logprob, 0);
}

// the same with sequences cut every block_rows rows (<= 0: the default; at least the longest sequence: one wave per sequence)
extern "C" int paa_debug_hmm_dev_decode_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                                            const int64_t *offsets, int64_t n_seq, int32_t *d_states, double *d_logprob,
                                            int64_t block_rows) {
    return hmm_dev_decode(handle, d_feats, n_dims, ld, n_vec, offsets, n_seq, d_states, d_logprob, block_rows);
}

extern "C" int paa_hmm_dev_loglik_f64(const void *handle, const double *d_feats, int n_dims, int64_t ld, int64_t n_vec,
                                      double *d_loglik) {
    int rc = model_check<PaaHmm>(handle, n_dims, ld, n_vec, kHmmMaxVec);
    if (rc) return rc;
    if (!d_feats || !d_loglik) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    LAUNCH_TRY("HMM emission",
               launch::hmm_emission(((const PaaHmm *)handle)->dev, d_feats, (long long)ld, (long long)n_vec, d_loglik, cs()));
    return PAA_OK;
}

extern "C" int paa_hmm_decode_f64(const void *handle, const double *feats, int n_dims, int64_t ld, int64_t n_vec,
                                  const int64_t *offsets, int64_t n_seq, int32_t *states, double *logprob) {
    int rc = model_check<PaaHmm>(handle, n_dims, ld, n_vec, kHmmMaxVec);
    if (rc) return rc;
    if ((rc = hmm_check_offsets(offsets, n_seq, n_vec))) return rc;
    if (!feats || !states || !logprob) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    Staged st;
    if ((rc = stage(st, feats, n_dims, ld, nullptr, nullptr, 0, {{states, (size_t)n_vec * 4}, {logprob, (size_t)n_seq * 8}}))) return rc;
    if ((rc = hmm_decode_core((PaaHmm *)handle, st.feats, ld, n_vec, offsets, n_seq, (int32_t *)st.out[0], (double *)st.out[1], 0)))
        return rc;
    return finish(st);
}

static int hmm_stats_check(int n_dims, int64_t ld, int64_t n_vec, const int32_t *labels, int n_states) {
    if (n_states < 1 || n_states > hmm::kMaxStates) return fail(PAA_ERR_ARG, "%d states: 1..%d are supported", n_states, hmm::kMaxStates);
    if (n_dims < 1 || n_dims > hmm::kMaxDims) return fail(PAA_ERR_ARG, "%d feature dimensions: 1..%d are supported", n_dims, hmm::kMaxDims);
    int rc = check_matrix(ld, n_vec, 0);
    if (rc) return rc;
    if (!labels) return fail(PAA_ERR_ARG, "null labels");
    for (int64_t t = 0; t < n_vec; ++t)
        if (labels[t] < 0 || labels[t] >= n_states)
            return fail(PAA_ERR_ARG, "label %d at %lld is outside 0..%d", labels[t], (long long)t, n_states - 1);
    return PAA_OK;
}

// synchronous on cs(); priors [K], transmat [K][K] (a row without transitions is 0 / 0 = NaN, as in the reference), means
// and covars (standard deviations) [K][n_dims] go to the host
static int hmm_stats_core(const double *d_feats, int n_dims, int64_t ld, int64_t n_vec, const int32_t *labels, int K,
                          double *priors, double *transmat, double *means, double *covars) {
    std::lock_guard<std::mutex> lk(g_hmm_stats_mu);
    const size_t b_lab = up256((size_t)n_vec * 4), cells = (size_t)K + (size_t)K * K, b_cnt = up256(cells * 4),
                 b_mom = up256((size_t)K * n_dims * 8);
    int rc = scratch_reserve(g_hmm_stats, b_lab + b_cnt + 2 * b_mom);
    if (rc) return rc;
    char *p = (char *)g_hmm_stats.p;
    int *d_labels = (int *)p;
    int *d_counts = (int *)(p + b_lab);
    double *d_means = (double *)(p + b_lab + b_cnt), *d_stds = (double *)(p + b_lab + b_cnt + b_mom);
    HIP_TRY(hipMemcpyAsync(d_labels, labels, (size_t)n_vec * 4, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemsetAsync(d_counts, 0, cells * 4, cs()));
    LAUNCH_TRY("HMM statistics",
               launch::hmm_stats(d_feats, (long long)ld, (long long)n_vec, d_labels, K, n_dims, d_counts, d_means, d_stds, cs()));
    std::vector<int> counts(cells);
    HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, cells * 4, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(means, d_means, (size_t)K * n_dims * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(covars, d_stds, (size_t)K * n_dims * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    double total = 0.0;
    for (int k = 0; k < K; ++k) total += (double)counts[k];
    for (int k = 0; k < K; ++k) priors[k] = (double)counts[k] / total;
    for (int a = 0; a < K; ++a) {
        double row = 0.0;
        for (int b = 0; b < K; ++b) row += (double)counts[K + a * K + b];
        for (int b = 0; b < K; ++b) transmat[a * K + b] = (double)counts[K + a * K + b] / row;
    }
    return PAA_OK;
}

extern "C" int paa_hmm_dev_train_stats_f64(const double *d_feats, int n_dims, int64_t ld, int64_t n_vec, const int32_t *labels,
                                           int n_states, double *priors, double *transmat, double *means, double *covars) {
    int rc = hmm_stats_check(n_dims, ld, n_vec, labels, n_states);
    if (rc) return rc;
    if (!d_feats || !priors || !transmat || !means || !covars) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    return hmm_stats_core(d_feats, n_dims, ld, n_vec, labels, n_states, priors, transmat, means, covars);
}

extern "C" int paa_hmm_train_stats_f64(const double *feats, int n_dims, int64_t ld, int64_t n_vec, const int32_t *labels,
                                       int n_states, double *priors, double *transmat, double *means, double *covars) {
    int rc = hmm_stats_check(n_dims, ld, n_vec, labels, n_states);
    if (rc) return rc;
    if (!feats || !priors || !transmat || !means || !covars) return fail(PAA_ERR_ARG, "null buffer");
    if ((rc = ensure_init())) return rc;
    Staged st;
    if ((rc = stage(st, feats, n_dims, ld, nullptr, nullptr, 0, {}))) return rc;
    return hmm_stats_core(st.feats, n_dims, ld, n_vec, labels, n_states, priors, transmat, means, covars);
}
