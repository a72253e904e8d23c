// Speaker diarization of a batch of clips (audioSegmentation.diarize_features_batch): the entry points of lib_diar.hpp over
// MANY clips that lie side by side in one device matrix.  prepare = standardisation + the all-window feature-row distances of
// every clip, one read-back; sweep = k-means++ seeding on the device, k-means over the (clip, k) job list, the per-cluster
// feature-row distances and the cluster-pair sums, with one wait per Lloyd iteration of the slowest job and a constant number
// besides.  Kernels: kernels_diarbatch.hpp (family_diar.hip).  Work space and lock are lib_diar.hpp's.
#pragma once
#include <chrono>

namespace diarb_host {

struct Blob {                           // host image of the record arrays, uploaded in one copy
    std::vector<char> bytes;
    template <typename T>
    size_t add(const std::vector<T> &v) {
        const size_t at = up256(bytes.size());
        bytes.resize(at + std::max<size_t>(v.size(), 1) * sizeof(T), 0);
        if (!v.empty()) std::memcpy(bytes.data() + at, v.data(), v.size() * sizeof(T));
        return at;
    }
};

static int check_clips(int n_dims, int64_t ld, int n_clips, const int64_t *cols, const int64_t *ns) {
    if (n_dims < 1 || n_dims > hmm::kMaxDims) return fail(PAA_ERR_ARG, "%d feature dimensions: 1..%d are supported", n_dims, hmm::kMaxDims);
    if (n_clips < 1 || n_clips > 65535) return fail(PAA_ERR_ARG, "%d clips: 1..65535 per call", n_clips);
    if (!cols || !ns || ld < 1) return fail(PAA_ERR_ARG, "null buffer");
    for (int i = 0; i < n_clips; ++i)
        if (ns[i] < 1 || ns[i] > 0x7fffffffLL / 64 || cols[i] < 0 || cols[i] + ns[i] > ld)
            return fail(PAA_ERR_ARG, "clip %d: windows %lld .. %lld of a matrix of %lld columns", i, (long long)cols[i],
                        (long long)(cols[i] + ns[i]), (long long)ld);
    return PAA_OK;
}

static double ms_since(std::chrono::steady_clock::time_point &t0) {
    const auto t1 = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
    return ms;
}

}  // namespace diarb_host

extern "C" int paa_diar_batch_prepare_f64(const double *d_feats, int n_dims, int64_t ld, const int64_t *cols, const int64_t *ns,
                                          int n_clips, double *d_z, double *stats, double *colsum) {
    int rc = diarb_host::check_clips(n_dims, ld, n_clips, cols, ns);
    if (rc) return rc;
    if (!d_feats || !d_z || !stats || !colsum) return fail(PAA_ERR_ARG, "null buffer");
    if (d_feats == d_z) return fail(PAA_ERR_ARG, "the standardised matrix needs a buffer of its own");
    if ((rc = ensure_init())) return rc;
    std::vector<diar::BatchClip> clips(n_clips);
    std::vector<diar::BatchSlot> slots(n_clips);
    for (int i = 0; i < n_clips; ++i) {
        clips[i] = diar::BatchClip{cols[i], ns[i], 0, n_dims, 0, 0, 0, 0, 0};
        slots[i] = diar::BatchSlot{cols[i], ns[i], -1, (long long)i * n_dims * n_dims, (long long)i * n_dims, n_dims, -1, 0, 0};
    }
    diarb_host::Blob blob;
    const size_t o_clips = blob.add(clips), o_slots = blob.add(slots);
    std::lock_guard<std::mutex> lk(g_diar_mu);
    const size_t b_blob = up256(blob.bytes.size()), b_stats = up256((size_t)n_clips * 3 * n_dims * 8),
                 b_dist = up256((size_t)n_clips * n_dims * n_dims * 8), b_col = up256((size_t)n_clips * n_dims * 8),
                 b_pm = up256((size_t)n_clips * 8);
    if ((rc = scratch_reserve(g_diar, b_blob + b_stats + b_dist + b_col + b_pm))) return rc;
    char *p = (char *)g_diar.p;
    const auto *d_clips = (const diar::BatchClip *)(p + o_clips);
    const auto *d_slots = (const diar::BatchSlot *)(p + o_slots);
    p += b_blob;
    double *d_stats = (double *)p;      p += b_stats;
    double *d_dist = (double *)p;       p += b_dist;
    double *d_col = (double *)p;        p += b_col;
    double *d_pm = (double *)p;
    HIP_TRY(hipMemcpyAsync(g_diar.p, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, cs()));
    LAUNCH_TRY("batched standardisation", launch::diarb_standardize(d_feats, ld, d_clips, n_clips, n_dims, d_z, d_stats, cs()));
    LAUNCH_TRY("batched feature-row distance",
               launch::diarb_dim_distances(d_z, ld, nullptr, d_slots, n_clips, n_dims, nullptr, d_dist, d_col, d_pm, cs()));
    HIP_TRY(hipMemcpyAsync(stats, d_stats, (size_t)n_clips * 3 * n_dims * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(colsum, d_col, (size_t)n_clips * n_dims * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}

extern "C" int paa_diar_batch_sweep_f64(const double *d_z, int n_dims, int64_t ld, int n_clips, const int64_t *cols, const int64_t *ns,
                                        const int32_t *dims, const int32_t *rows, const int32_t *nks, const int32_t *ks,
                                        const double *tols, int max_iter, const int32_t *seeded, const int64_t *first,
                                        const double *u, double *centers, int32_t *d_labels, int32_t *n_iter, double *inertia,
                                        double *a_mean, double *pair_sums, double *stage_ms) {
    int rc = diarb_host::check_clips(n_dims, ld, n_clips, cols, ns);
    if (rc) return rc;
    if (!d_z || !dims || !rows || !nks || !ks || !tols || !seeded || !first || !centers || !d_labels || !n_iter || !inertia || !a_mean ||
        !pair_sums)
        return fail(PAA_ERR_ARG, "null buffer");
    if (max_iter < 1) return fail(PAA_ERR_ARG, "max_iter %d", max_iter);
    const int W = hmm::kMaxStates;
    std::vector<diar::BatchClip> clips(n_clips);
    std::vector<diar::BatchJob> jobs;
    std::vector<diar::BatchSlot> slots;
    std::vector<diar::BatchTile> items;
    std::vector<diar::BatchRed> red1, red2;
    std::vector<int> bintab, slot_job;
    long long n_rows = 0, L = 0, tmp_len = 0, u_len = 0, cen_len = 0, dist_len = 0, sum_len = 0, part_len = 0, stage_len = 0, S_len = 0,
              max_n = 0;
    int kmax = 0, max_D = 0, max_bins = 0, any_seeded = 0;
    for (int i = 0; i < n_clips; ++i) {
        const int D = dims[i], nk = nks[i];
        const long long n = ns[i];
        if (D < 1 || D > n_dims) return fail(PAA_ERR_ARG, "clip %d: %d kept rows of %d", i, D, n_dims);
        for (int d = 0; d < D; ++d)
            if (rows[n_rows + d] < 0 || rows[n_rows + d] >= n_dims) return fail(PAA_ERR_ARG, "clip %d: row %d is outside 0..%d", i, rows[n_rows + d], n_dims - 1);
        if (nk < 1 || nk > W) return fail(PAA_ERR_ARG, "clip %d: a sweep has 1..%d cluster counts", i, W);
        if (!(tols[i] >= 0.0)) return fail(PAA_ERR_ARG, "clip %d: tol %g", i, tols[i]);
        diar::BatchClip &cl = clips[i];
        cl = diar::BatchClip{cols[i], n, L, D, (int)n_rows, (int)jobs.size(), nk, (int)bintab.size(), 0};
        int nbins = 0;
        for (int j = 0; j < nk; ++j) {
            const int job = (int)jobs.size(), k = ks[job];
            if (k < 1 || k > W) return fail(PAA_ERR_ARG, "clip %d: %d clusters: 1..%d are supported", i, k, W);
            if (k > n) return fail(PAA_ERR_ARG, "clip %d: %d clusters for %lld vectors", i, k, (long long)n);
            diar::BatchJob jb{};
            jb.col = cols[i];
            jb.n = n;
            jb.lab_off = L;
            jb.cen_off = cen_len;
            jb.tol = tols[i];
            jb.D = D;
            jb.rows_off = (int)n_rows;
            jb.k = k;
            jb.seeded = seeded[job] ? 1 : 0;
            jb.trials = 2 + (int)std::log((double)k);
            if (jb.seeded) {
                if (!u) return fail(PAA_ERR_ARG, "null buffer");
                if (first[job] < 0 || first[job] >= n) return fail(PAA_ERR_ARG, "clip %d: first window %lld is outside 0..%lld", i, (long long)first[job], (long long)n - 1);
                jb.first = first[job];
                jb.tmp_off = tmp_len;
                jb.u_off = u_len;
                tmp_len += (long long)jb.trials * n;
                u_len += (long long)(k - 1) * jb.trials;
                any_seeded = 1;
            } else {
                for (long long e = 0; e < (long long)k * D; ++e)
                    if (!std::isfinite(centers[cen_len + e])) return fail(PAA_ERR_ARG, "clip %d: an initial centre is not finite", i);
            }
            for (int c = 0; c < k; ++c) {
                slots.push_back(diar::BatchSlot{cols[i], n, L, dist_len, sum_len, D, (int)n_rows, c, 0});
                slot_job.push_back(job);
                dist_len += (long long)D * D;
                sum_len += D;
            }
            bintab.push_back(nbins);
            nbins += k * k;
            L += n;
            cen_len += (long long)k * D;
            kmax = std::max(kmax, k);
            jobs.push_back(jb);
        }
        bintab.push_back(nbins);
        const long long nb = (n + diar::kBatchPairTile - 1) / diar::kBatchPairTile, tiles = nb * (nb + 1) / 2,
                        chunks = (tiles + launch::kDiarbPairChunk - 1) / launch::kDiarbPairChunk;
        if (tiles + (long long)items.size() > 0x7fffffffLL) return fail(PAA_ERR_ARG, "too many window pairs for one call");
        const long long part0 = part_len;
        for (long long bi = 0; bi < nb; ++bi)
            for (long long bj = bi; bj < nb; ++bj) {
                items.push_back(diar::BatchTile{part_len, i, (int)bi, (int)bj, 0});
                part_len += nbins;
            }
        for (long long c = 0; c < chunks; ++c) {
            const long long r0 = c * launch::kDiarbPairChunk, r1 = std::min(r0 + launch::kDiarbPairChunk, tiles);
            red1.push_back(diar::BatchRed{part0 + r0 * nbins, r1 - r0, stage_len + c * nbins, nbins, 0});
        }
        red2.push_back(diar::BatchRed{stage_len, chunks, S_len, nbins, 0});
        stage_len += chunks * nbins;
        S_len += nbins;
        n_rows += D;
        max_n = std::max(max_n, n);
        max_D = std::max(max_D, D);
        max_bins = std::max(max_bins, nbins);
    }
    const int n_jobs = (int)jobs.size(), n_slots = (int)slots.size();
    if (n_jobs > 65535 || n_slots > 65535 || red1.size() > 65535) return fail(PAA_ERR_ARG, "%d jobs and %d clusters: at most 65535 per call", n_jobs, n_slots);
    for (long long e = 0; e < u_len; ++e)
        if (!(u[e] >= 0.0 && u[e] < 1.0)) return fail(PAA_ERR_ARG, "a seeding draw is outside [0, 1)");
    if ((rc = ensure_init())) return rc;
    diarb_host::Blob blob;
    const std::vector<int> rows_v(rows, rows + n_rows);
    const std::vector<double> u_v(u ? u : nullptr, u ? u + u_len : nullptr);
    const size_t o_clips = blob.add(clips), o_jobs = blob.add(jobs), o_slots = blob.add(slots), o_items = blob.add(items),
                 o_red1 = blob.add(red1), o_red2 = blob.add(red2), o_rows = blob.add(rows_v), o_bintab = blob.add(bintab),
                 o_u = blob.add(u_v);
    std::lock_guard<std::mutex> lk(g_diar_mu);
    const size_t b_blob = up256(blob.bytes.size()), b_cen = up256((size_t)cen_len * 8), b_state = up256((size_t)n_jobs * sizeof(diar::KmState)),
                 b_d2 = up256((size_t)L * 8), b_tmp = up256((size_t)std::max<long long>(tmp_len, 1) * 8),
                 b_ints = up256((size_t)n_jobs * diar::kIntsPerK * 4), b_in = up256((size_t)n_jobs * 8),
                 b_dist = up256((size_t)dist_len * 8), b_sum = up256((size_t)sum_len * 8), b_pm = up256((size_t)n_slots * 8),
                 b_part = up256((size_t)part_len * 8), b_stage = up256((size_t)stage_len * 8), b_S = up256((size_t)S_len * 8);
    if ((rc = scratch_reserve(g_diar, b_blob + 2 * b_cen + b_state + b_d2 + b_tmp + b_ints + b_in + b_dist + b_sum + b_pm + b_part +
                                          b_stage + b_S)))
        return rc;
    char *p = (char *)g_diar.p;
    const auto *d_clips = (const diar::BatchClip *)(p + o_clips);
    const auto *d_jobs = (const diar::BatchJob *)(p + o_jobs);
    const auto *d_slots = (const diar::BatchSlot *)(p + o_slots);
    const auto *d_items = (const diar::BatchTile *)(p + o_items);
    const auto *d_red1 = (const diar::BatchRed *)(p + o_red1), *d_red2 = (const diar::BatchRed *)(p + o_red2);
    const int *d_rows = (const int *)(p + o_rows), *d_bintab = (const int *)(p + o_bintab);
    const double *d_u = (const double *)(p + o_u);
    p += b_blob;
    double *d_cen = (double *)p;                            p += b_cen;
    double *d_sums = (double *)p;                           p += b_cen;
    diar::KmState *d_state = (diar::KmState *)p;            p += b_state;
    double *d_d2 = (double *)p;                             p += b_d2;
    double *d_tmp = (double *)p;                            p += b_tmp;
    int *d_ints = (int *)p;                                 p += b_ints;
    double *d_inertia = (double *)p;                        p += b_in;
    double *d_dist = (double *)p;                           p += b_dist;
    double *d_sum = (double *)p;                            p += b_sum;
    double *d_pm = (double *)p;                             p += b_pm;
    double *d_part = (double *)p;                           p += b_part;
    double *d_stage = (double *)p;                          p += b_stage;
    double *d_S = (double *)p;
    auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpyAsync(g_diar.p, blob.bytes.data(), blob.bytes.size(), hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemcpyAsync(d_cen, centers, (size_t)cen_len * 8, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemsetAsync(d_sums, 0, (size_t)cen_len * 8, cs()));
    HIP_TRY(hipMemsetAsync(d_state, 0, (size_t)n_jobs * sizeof(diar::KmState), cs()));
    HIP_TRY(hipMemsetAsync(d_labels, 0xff, (size_t)L * 4, cs()));       // -1: no window keeps its label in iteration 1
    // the seeding's closest distances live in d2 until the first assignment overwrites them
    if (any_seeded) LAUNCH_TRY("k-means++ seeding", launch::diarb_seed(d_z, ld, d_rows, d_jobs, n_jobs, d_u, d_d2, d_tmp, d_cen, cs()));
    if (stage_ms) {
        HIP_TRY(hipStreamSynchronize(cs()));
        stage_ms[0] = diarb_host::ms_since(t0);
    }
    std::vector<diar::KmState> state(n_jobs);
    int rounds = 0;
    for (int it = 0; it < max_iter; ++it) {
        LAUNCH_TRY("batched k-means", launch::diarb_kmeans_step(d_z, ld, d_rows, d_jobs, n_jobs, kmax, max_n, max_D, d_cen, d_state,
                                                                d_labels, d_d2, d_ints, d_sums, max_iter, cs()));
        HIP_TRY(hipMemcpyAsync(state.data(), d_state, (size_t)n_jobs * sizeof(diar::KmState), hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipStreamSynchronize(cs()));
        ++rounds;
        bool all = true;
        for (int i = 0; i < n_jobs; ++i) all = all && state[i].done;
        if (all) break;
    }
    LAUNCH_TRY("batched k-means",
               launch::diarb_kmeans_last(d_z, ld, d_rows, d_jobs, n_jobs, kmax, max_n, d_cen, d_state, d_labels, d_d2, d_inertia, cs()));
    if (stage_ms) {
        HIP_TRY(hipStreamSynchronize(cs()));
        stage_ms[1] = diarb_host::ms_since(t0);
        stage_ms[3] = (double)rounds;
    }
    LAUNCH_TRY("batched feature-row distance",
               launch::diarb_dim_distances(d_z, ld, d_rows, d_slots, n_slots, max_D, d_labels, d_dist, d_sum, d_pm, cs()));
    LAUNCH_TRY("batched cluster-pair",
               launch::diarb_pair_sums(d_z, ld, d_rows, d_clips, d_jobs, d_items, (int)items.size(), d_labels, d_bintab, d_part, d_red1,
                                       (int)red1.size(), d_stage, d_red2, (int)red2.size(), d_S, max_bins, 2 * g_num_cu, cs()));
    std::vector<double> pm(n_slots), flat((size_t)S_len);
    HIP_TRY(hipMemcpyAsync(centers, d_cen, (size_t)cen_len * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(inertia, d_inertia, (size_t)n_jobs * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(pm.data(), d_pm, (size_t)n_slots * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(flat.data(), d_S, (size_t)S_len * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    if (stage_ms) stage_ms[2] = diarb_host::ms_since(t0);
    std::fill(a_mean, a_mean + (size_t)n_jobs * W, 0.0);
    std::fill(pair_sums, pair_sums + (size_t)n_jobs * W * W, 0.0);
    for (int s = 0; s < n_slots; ++s) a_mean[(size_t)slot_job[s] * W + slots[s].cluster] = pm[s];
    long long S_at = 0;
    for (int i = 0; i < n_clips; ++i) {
        const int *bt = bintab.data() + clips[i].bin_tab;
        for (int j = 0; j < clips[i].nk; ++j) {
            const int job = clips[i].first_job + j, k = jobs[job].k;
            n_iter[job] = state[job].n_iter;
            for (int c = 0; c < k; ++c)
                for (int c2 = 0; c2 < k; ++c2) pair_sums[((size_t)job * W + c) * W + c2] = flat[S_at + bt[j] + c * k + c2];
        }
        S_at += bt[clips[i].nk];
    }
    return PAA_OK;
}

extern "C" int paa_diar_batch_gather_f64(const double *d_slabs, int n_rows, const int64_t *slab_offsets, const int64_t *cols,
                                         const int64_t *ns, int n_clips, double *d_out, int64_t ld) {
    int rc = diarb_host::check_clips(n_rows, ld, n_clips, cols, ns);
    if (rc) return rc;
    if (!d_slabs || !slab_offsets || !d_out) return fail(PAA_ERR_ARG, "null buffer");
    for (int i = 0; i < n_clips; ++i)
        if (slab_offsets[i] < 0) return fail(PAA_ERR_ARG, "clip %d: slab offset %lld", i, (long long)slab_offsets[i]);
    if ((rc = ensure_init())) return rc;
    for (int i = 0; i < n_clips; ++i)
        HIP_TRY(hipMemcpy2DAsync(d_out + cols[i], (size_t)ld * 8, d_slabs + slab_offsets[i], (size_t)ns[i] * 8, (size_t)ns[i] * 8,
                                 (size_t)n_rows, hipMemcpyDeviceToDevice, cs()));
    return PAA_OK;
}
