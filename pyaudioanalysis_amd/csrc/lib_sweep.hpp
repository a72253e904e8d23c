// What the sweeps over index lists into ONE resident sample matrix share on the host (lib_knn.hpp: paa_knn_splits_f64;
// lib_smo.hpp: paa_smo_tasks_f64, paa_svc_fit_splits_f64): the argument checks of the matrix, the offset arrays and the index
// lists, and the table of workgroups over the test lists.  Every check runs before ensure_init().  No device code.
#pragma once

constexpr int64_t kSweepMaxQ = 0x7fffffffLL;        // a test vector's place in the outputs is an int32 on the host side of the table

static int sweep_samples_check(int64_t n_samples) {
    if (n_samples < 1 || n_samples > 0x7fffffffLL) return fail(PAA_ERR_ARG, "%lld samples", (long long)n_samples);
    return PAA_OK;
}

// offsets [n + 1] from 0 and not decreasing, no list longer than an int; `what`: "train", "test", "task"
static int sweep_offsets_check(const int64_t *off, int n, const char *what) {
    if (off[0] != 0) return fail(PAA_ERR_ARG, "%s offsets begin at %lld, not 0", what, (long long)off[0]);
    for (int j = 0; j < n; ++j)
        if (off[j + 1] < off[j] || off[j + 1] - off[j] > 0x7fffffffLL)
            return fail(PAA_ERR_ARG, "%s offsets of job %d: %lld .. %lld", what, j, (long long)off[j], (long long)off[j + 1]);
    return PAA_OK;
}

// the jobs of a split sweep: at least one, both offset arrays, no more test vectors than the outputs can index
static int sweep_jobs_check(int n_jobs, const int64_t *train_off, const int64_t *test_off) {
    if (n_jobs < 1) return fail(PAA_ERR_ARG, "no jobs");
    int rc;
    if ((rc = sweep_offsets_check(train_off, n_jobs, "train"))) return rc;
    if ((rc = sweep_offsets_check(test_off, n_jobs, "test"))) return rc;
    if (test_off[n_jobs] > kSweepMaxQ) return fail(PAA_ERR_ARG, "too many test vectors");
    return PAA_OK;
}

// every index of a list is a row of the sample matrix; `what`: "train", "test", "row"
static int sweep_index_check(const int32_t *idx, int64_t n, int64_t n_samples, const char *what) {
    for (int64_t i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= n_samples) return fail(PAA_ERR_ARG, "%s index %d of %lld samples", what, idx[i], (long long)n_samples);
    return PAA_OK;
}

// the grid over the test lists: per job one workgroup for every `per_block` of its test vectors (knn::kQueriesPerBlock,
// smo::kQueriesPerBlock), job after job
static std::vector<knn::SplitBlock> sweep_blocks(const int64_t *test_off, int n_jobs, int per_block) {
    std::vector<knn::SplitBlock> blocks;
    for (int j = 0; j < n_jobs; ++j)
        for (int64_t first = 0; first < test_off[j + 1] - test_off[j]; first += per_block) blocks.push_back({j, (int)first});
    return blocks;
}
