// The SVR fits of audioTrainTest.evaluate_regression (audioTrainTest.py:774-855 with train_svm_regression :222-226) on the device:
// a batch of epsilon-SVR dual problems (tasks) over ONE uploaded sample matrix and its targets, solved by relaunching
// svr_smo_kernel until every task has stopped (smo_relaunch_some, lib_smo.hpp), and the split sweep built on it: one task per job,
// then svc_pairs_kernel over the test rows, a job being one "pair" whose alpha_y is beta -- its decision value is the prediction.
// With a resident kernel matrix (DESIGN K22, the *_cached_f64 entry points) the tasks are packed into chunks whose n x n matrices fit
// `cache_bytes`; per chunk: svr_standardise_kernel, svr_gram_kernel, then smo_relaunch_some with svr_smo_cached_kernel, then the
// scratch serves the next chunk (lib_gramcache.hpp).  A task whose matrix alone exceeds the budget goes to svr_smo_kernel in the same call.
// Kernels: kernels_svrfit.hpp and kernels_svrcache.hpp (family_svr.hip), kernels_smo.hpp (family_smo.hip).
#pragma once

// what a task adds to smo_task_check: the width of its tube
static int svr_epsilon_check(int t, double epsilon) {
    if (!(epsilon >= 0.0) || !std::isfinite(epsilon)) return fail(PAA_ERR_ARG, "task %d: epsilon = %g", t, epsilon);
    return PAA_OK;
}
static int svr_targets_check(const double *y, int64_t n_samples) {
    for (int64_t i = 0; i < n_samples; ++i)
        if (!std::isfinite(y[i])) return fail(PAA_ERR_ARG, "the target of sample %lld is %g", (long long)i, y[i]);
    return PAA_OK;
}

// The state of a batch on the device, freed on return: alpha | G [2 rows]; QD | beta | train_pred [rows]; rho | gap [tasks]; iter |
// status | n_sv | live [tasks]; label [n_q] (what svc_pairs_kernel writes beside the decision values)
struct SvrFitState {
    DevBlock block;
    int *live = nullptr, *label = nullptr;
};
static int svr_state_alloc(SvrFitState &s, svrfit::SvrDev &m, size_t rows, size_t n_tasks, size_t n_q) {
    const size_t b_rows = up256(rows * 8), b_task8 = up256(n_tasks * 8), b_task4 = up256(n_tasks * 4);
    HIP_TRY(hipMalloc(&s.block.p, 7 * b_rows + 2 * b_task8 + 4 * b_task4 + up256(n_q * 4)));
    char *p = (char *)s.block.p;
    m.alpha = (double *)p;      p += 2 * b_rows;
    m.G = (double *)p;          p += 2 * b_rows;
    m.QD = (double *)p;         p += b_rows;
    m.beta = (double *)p;       p += b_rows;
    m.train_pred = (double *)p; p += b_rows;
    m.rho = (double *)p;        p += b_task8;
    m.gap = (double *)p;        p += b_task8;
    m.iter = (int *)p;          p += b_task4;
    m.status = (int *)p;        p += b_task4;
    m.n_sv = (int *)p;          p += b_task4;
    s.live = (int *)p;          p += b_task4;
    s.label = (int *)p;
    HIP_TRY(hipMemsetAsync(m.iter, 0, 2 * b_task4, cs()));       // iteration 0, status kFresh
    return PAA_OK;
}

// The steps of smo_relaunch_some: svr_smo_kernel, and svr_smo_cached_kernel over the resident matrices c, for the tasks listed in `live`
struct SvrStep {
    const svrfit::SvrDev &m;
    const int *live;
    int operator()(int n_live, int n_max, int budget) const {
        LAUNCH_TRY("SVR SMO", launch::svr_smo_step(m, live, n_live, n_max, budget, cs()));
        return PAA_OK;
    }
};
struct SvrCachedStep {
    const svrfit::SvrDev &m;
    const svrfit::SvrCacheDev &c;
    const int *live;
    int operator()(int n_live, int n_max, int budget) const {
        LAUNCH_TRY("cached SVR SMO", launch::svr_smo_cached_step(m, c, live, n_live, n_max, budget, cs()));
        return PAA_OK;
    }
};

// Solves a batch: allocates its state into s and m, then runs every task to its stop (smo_relaunch_some), from resident matrices
// under the budget cache_bytes where they fit; cached [tasks] (may be null): 1 for a task solved from its matrix.  cache_bytes = 0 is
// "no cache": no matrix fits, no chunk is formed and every task goes to svr_smo_kernel in one relaunch loop
static int svr_solve_batch(svrfit::SvrDev &m, SvrFitState &s, const std::vector<smo::SmoTask> &tasks, size_t rows, size_t n_q,
                           int iters_per_launch, std::vector<int> &status, int *n_launches, int64_t cache_bytes, int32_t *cached) {
    int rc;
    if ((rc = svr_state_alloc(s, m, rows, tasks.size(), n_q))) return rc;
    SvrCache c;
    if ((rc = svr_cache_alloc(c, tasks, m.n_dims, cache_bytes))) return rc;
    status.assign(tasks.size(), smo::kFresh);
    long long launches = 0;
    std::vector<int> members;
    for (size_t t = 0; t < tasks.size(); ++t) {
        if (cached) cached[t] = c.chunk_of[t] >= 0;
        if (c.chunk_of[t] < 0) members.push_back((int)t);
    }
    if (!members.empty() &&
        (rc = smo_relaunch_some(tasks, members, m.max_iter, iters_per_launch, s.live, m.status, status, launches, SvrStep{m, s.live})))
        return rc;
    for (int ch = 0; ch < c.n_chunks; ++ch) {
        if ((rc = svr_cache_fill(c, m, tasks, ch, members))) return rc;
        if ((rc = smo_relaunch_some(tasks, members, m.max_iter, iters_per_launch, s.live, m.status, status, launches,
                                    SvrCachedStep{m, c.dev, s.live})))
            return rc;
    }
    if (n_launches) *n_launches = (int)launches;
    return PAA_OK;
}

// the solver's view of an uploaded batch: the staged matrix, the uploaded y | tasks | epsilon | mean | scale | idx and the parameters
static svrfit::SvrDev svr_dev(const double *X, const BlockPart &y, const BlockPart &tasks, const BlockPart &epsilon, const BlockPart &mean,
                              const BlockPart &scale, const BlockPart &idx, int n_dims, int kernel_type, double eps, int max_iter) {
    svrfit::SvrDev m{};
    m.X = X;
    m.y = (const double *)y.dev;
    m.tasks = (const smo::SmoTask *)tasks.dev;
    m.epsilon = (const double *)epsilon.dev;
    m.mean = (const double *)mean.dev;
    m.scale = (const double *)scale.dev;
    m.idx = (const int *)idx.dev;
    m.n_dims = n_dims;
    m.rbf = kernel_type == 2;
    m.max_iter = max_iter;
    m.eps = eps;
    return m;
}

// the tasks of index lists list_off [n + 1]: task t is list t with the statistics row t; every check of a task
static int svr_tasks(std::vector<smo::SmoTask> &tasks, int n, const int64_t *list_off, const double *C, const double *gamma,
                     const double *epsilon, int kernel_type) {
    tasks.resize(n);
    for (int t = 0; t < n; ++t) {
        int rc;
        if ((rc = smo_task_check(t, list_off[t + 1] - list_off[t], C[t], gamma[t], kernel_type))) return rc;
        if ((rc = svr_epsilon_check(t, epsilon[t]))) return rc;
        tasks[t] = {(long long)list_off[t], (int)(list_off[t + 1] - list_off[t]), t, C[t], gamma[t]};
    }
    return PAA_OK;
}

// The solver alone (libsvm's solve_epsilon_svr over Solver::Solve, svm.cpp, as svm_train_one runs it under SVR.fit): see paa_hip.h
// (use_cache false: paa_svr_tasks_f64; true: paa_svr_tasks_cached_f64 with its budget and flags)
static int svr_tasks_run(const double *X, int64_t n_samples, int n_dims, const double *y, int n_tasks, const int64_t *task_off,
                         const int32_t *task_idx, const double *mean, const double *std, const double *C, const double *gamma,
                         const double *epsilon, int kernel_type, double eps, int max_iter, int iters_per_launch, double *beta, double *rho,
                         int32_t *iterations, double *gap, int32_t *status, int32_t *n_sv, double *train_pred, int32_t *n_launches,
                         bool use_cache, int64_t cache_bytes, int32_t *cached) {
    if (!X || !y || !task_off || !task_idx || !mean || !std || !C || !gamma || !epsilon || !beta || !rho || !iterations || !gap || !status ||
        !n_sv || !train_pred || (use_cache && !cached))
        return fail(PAA_ERR_ARG, "null argument");
    int rc;
    if ((rc = sweep_samples_check(n_samples))) return rc;
    if ((rc = smo_params_check(n_dims, kernel_type, eps, max_iter, iters_per_launch))) return rc;
    if (n_tasks < 1) return fail(PAA_ERR_ARG, "no tasks");
    if ((rc = sweep_offsets_check(task_off, n_tasks, "task"))) return rc;
    const int64_t rows = task_off[n_tasks];
    std::vector<smo::SmoTask> tasks;
    if ((rc = svr_tasks(tasks, n_tasks, task_off, C, gamma, epsilon, kernel_type))) return rc;
    if ((rc = sweep_index_check(task_idx, rows, n_samples, "row"))) return rc;
    if ((rc = svr_targets_check(y, n_samples))) return rc;
    if (use_cache && (rc = svr_cache_args_check(cache_bytes))) return rc;
    if ((rc = ensure_init())) return rc;
    const size_t sb = (size_t)n_tasks * n_dims * 8;
    DevBlock block;
    BlockPart parts[] = {{y, (size_t)n_samples * 8, 8}, {tasks.data(), tasks.size() * sizeof(smo::SmoTask), 8}, {epsilon, (size_t)n_tasks * 8, 8},
                         {mean, sb, 8}, {std, sb, 8}, {task_idx, (size_t)rows * 4, 4}};
    if ((rc = block_upload(block, parts, 6, "the SVR tasks"))) return rc;
    Staged st;                                        // X goes up once, through the lane's scratch
    if ((rc = stage(st, X, n_dims, n_samples, nullptr, nullptr, 0, {}))) return rc;
    svrfit::SvrDev m = svr_dev(st.feats, parts[0], parts[1], parts[2], parts[3], parts[4], parts[5], n_dims, kernel_type, eps, max_iter);
    SvrFitState s;
    std::vector<int> st_words;
    if ((rc = svr_solve_batch(m, s, tasks, (size_t)rows, 0, iters_per_launch, st_words, n_launches, use_cache ? cache_bytes : 0, cached)))
        return rc;
    HIP_TRY(hipMemcpyAsync(beta, m.beta, (size_t)rows * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(train_pred, m.train_pred, (size_t)rows * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(rho, m.rho, (size_t)n_tasks * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(gap, m.gap, (size_t)n_tasks * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(iterations, m.iter, (size_t)n_tasks * 4, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(n_sv, m.n_sv, (size_t)n_tasks * 4, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    std::copy(st_words.begin(), st_words.end(), status);
    return PAA_OK;
}
extern "C" int paa_svr_tasks_f64(const double *X, int64_t n_samples, int n_dims, const double *y, int n_tasks, const int64_t *task_off,
                                 const int32_t *task_idx, const double *mean, const double *std, const double *C, const double *gamma,
                                 const double *epsilon, int kernel_type, double eps, int max_iter, int iters_per_launch, double *beta,
                                 double *rho, int32_t *iterations, double *gap, int32_t *status, int32_t *n_sv, double *train_pred,
                                 int32_t *n_launches) {
    return svr_tasks_run(X, n_samples, n_dims, y, n_tasks, task_off, task_idx, mean, std, C, gamma, epsilon, kernel_type, eps, max_iter,
                         iters_per_launch, beta, rho, iterations, gap, status, n_sv, train_pred, n_launches, false, 0, nullptr);
}
extern "C" int paa_svr_tasks_cached_f64(const double *X, int64_t n_samples, int n_dims, const double *y, int n_tasks, const int64_t *task_off,
                                        const int32_t *task_idx, const double *mean, const double *std, const double *C, const double *gamma,
                                        const double *epsilon, int kernel_type, double eps, int max_iter, int iters_per_launch, double *beta,
                                        double *rho, int32_t *iterations, double *gap, int32_t *status, int32_t *n_sv, double *train_pred,
                                        int32_t *n_launches, int64_t cache_bytes, int32_t *cached) {
    return svr_tasks_run(X, n_samples, n_dims, y, n_tasks, task_off, task_idx, mean, std, C, gamma, epsilon, kernel_type, eps, max_iter,
                         iters_per_launch, beta, rho, iterations, gap, status, n_sv, train_pred, n_launches, true, cache_bytes, cached);
}

// The matrices alone (svr_standardise_kernel, svr_gram_kernel) of a task list, all in one chunk, and on request the K_tt that
// svr_smo_kernel itself forms at a task's start: see paa_hip.h
extern "C" int paa_svr_gram_f64(const double *X, int64_t n_samples, int n_dims, int n_tasks, const int64_t *task_off, const int32_t *task_idx,
                                const double *mean, const double *std, const double *gamma, int kernel_type, double *K_out, double *qd_out) {
    if (!X || !task_off || !task_idx || !mean || !std || !gamma || !K_out) return fail(PAA_ERR_ARG, "null argument");
    int rc;
    if ((rc = sweep_samples_check(n_samples))) return rc;
    if ((rc = smo_params_check(n_dims, kernel_type, 1.0, 1, 0))) return rc;
    if (n_tasks < 1) return fail(PAA_ERR_ARG, "no tasks");
    if ((rc = sweep_offsets_check(task_off, n_tasks, "task"))) return rc;
    const int64_t rows = task_off[n_tasks];
    std::vector<smo::SmoTask> tasks(n_tasks);
    for (int t = 0; t < n_tasks; ++t) {
        if ((rc = smo_task_check(t, task_off[t + 1] - task_off[t], 1.0, gamma[t], kernel_type))) return rc;
        tasks[t] = {(long long)task_off[t], (int)(task_off[t + 1] - task_off[t]), t, 1.0, gamma[t]};
    }
    if ((rc = sweep_index_check(task_idx, rows, n_samples, "row"))) return rc;
    if ((rc = ensure_init())) return rc;
    // zero targets and a zero tube: svr_smo_kernel forms K_tt, finds no violating pair and stops
    const std::vector<double> zeros((size_t)std::max<int64_t>(n_samples, n_tasks), 0.0);
    const size_t sb = (size_t)n_tasks * n_dims * 8;
    DevBlock block;
    BlockPart parts[] = {{zeros.data(), (size_t)n_samples * 8, 8}, {tasks.data(), tasks.size() * sizeof(smo::SmoTask), 8},
                         {zeros.data(), (size_t)n_tasks * 8, 8}, {mean, sb, 8}, {std, sb, 8}, {task_idx, (size_t)rows * 4, 4}};
    if ((rc = block_upload(block, parts, 6, "the SVR tasks"))) return rc;
    Staged st;
    if ((rc = stage(st, X, n_dims, n_samples, nullptr, nullptr, 0, {}))) return rc;
    svrfit::SvrDev m = svr_dev(st.feats, parts[0], parts[1], parts[2], parts[3], parts[4], parts[5], n_dims, kernel_type, 1.0, 1);
    SvrFitState s;
    if ((rc = svr_state_alloc(s, m, (size_t)rows, tasks.size(), 0))) return rc;
    SvrCache c;
    if ((rc = svr_cache_alloc(c, tasks, n_dims, INT64_MAX))) return rc;
    std::vector<int> members;
    if ((rc = svr_cache_fill(c, m, tasks, 0, members))) return rc;
    for (int t = 0; t < n_tasks; ++t) {
        const size_t n = (size_t)tasks[t].n;
        HIP_TRY(hipMemcpyAsync(K_out, c.dev.K + c.off[t], n * n * 8, hipMemcpyDeviceToHost, cs()));
        K_out += n * n;
    }
    if (qd_out) {
        std::vector<int> st_words(n_tasks, smo::kFresh);
        long long launches = 0;
        if ((rc = smo_relaunch_some(tasks, members, 1, 1, s.live, m.status, st_words, launches, SvrStep{m, s.live}))) return rc;
        HIP_TRY(hipMemcpyAsync(qd_out, m.QD, (size_t)rows * 8, hipMemcpyDeviceToHost, cs()));
    }
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}

// The SVR half of audioTrainTest.evaluate_regression (audioTrainTest.py:774-855): every split a job, every job one task over its
// training list; see paa_hip.h
// (use_cache false: paa_svr_fit_splits_f64; true: paa_svr_fit_splits_cached_f64 with its budget and flags)
static int svr_fit_splits_run(const double *X, int64_t n_samples, int n_dims, const double *y, int n_jobs, const int64_t *train_off,
                              const int32_t *train_idx, const int64_t *test_off, const int32_t *test_idx, const double *mean,
                              const double *std, const double *C, const double *gamma, const double *epsilon, int kernel_type, double eps,
                              int max_iter, int iters_per_launch, double *pred_out, double *train_pred_out, int32_t *job_iterations,
                              int32_t *job_status, int32_t *job_n_sv, int32_t *n_launches, bool use_cache, int64_t cache_bytes,
                              int32_t *cached) {
    // check
    if (!X || !y || !train_off || !train_idx || !test_off || !test_idx || !mean || !std || !C || !gamma || !epsilon || !pred_out ||
        (use_cache && !cached))
        return fail(PAA_ERR_ARG, "null argument");
    int rc;
    if ((rc = sweep_samples_check(n_samples))) return rc;
    if ((rc = smo_params_check(n_dims, kernel_type, eps, max_iter, iters_per_launch))) return rc;
    if ((rc = sweep_jobs_check(n_jobs, train_off, test_off))) return rc;
    const int64_t n_q = test_off[n_jobs], n_t = train_off[n_jobs];
    if ((rc = sweep_index_check(train_idx, n_t, n_samples, "train"))) return rc;
    if ((rc = sweep_index_check(test_idx, n_q, n_samples, "test"))) return rc;
    std::vector<smo::SmoTask> tasks;
    if ((rc = svr_tasks(tasks, n_jobs, train_off, C, gamma, epsilon, kernel_type))) return rc;
    if ((rc = svr_targets_check(y, n_samples))) return rc;
    if (use_cache && (rc = svr_cache_args_check(cache_bytes))) return rc;
    if ((rc = ensure_init())) return rc;
    // upload: a job is the one pair of two "classes" for the scoring kernel, its task the job's own number
    const std::vector<knn::SplitBlock> blocks = sweep_blocks(test_off, n_jobs, smo::kQueriesPerBlock);
    std::vector<int> job_task(n_jobs + 1), job_k(n_jobs, 2);
    for (int j = 0; j <= n_jobs; ++j) job_task[j] = j;
    const size_t sb = (size_t)n_jobs * n_dims * 8;
    const knn::SplitBlock none{0, 0};
    DevBlock block;
    BlockPart parts[] = {{y, (size_t)n_samples * 8, 8},
                         {tasks.data(), tasks.size() * sizeof(smo::SmoTask), 8},
                         {epsilon, (size_t)n_jobs * 8, 8},
                         {mean, sb, 8},
                         {std, sb, 8},
                         {test_off, (size_t)(n_jobs + 1) * 8, 8},
                         {blocks.empty() ? &none : blocks.data(), std::max<size_t>(blocks.size(), 1) * sizeof(knn::SplitBlock), 8},
                         {train_idx, (size_t)n_t * 4, 4},
                         {n_q ? test_idx : train_idx, (size_t)std::max<int64_t>(n_q, 1) * 4, 4},
                         {job_task.data(), (size_t)(n_jobs + 1) * 4, 4},
                         {job_k.data(), (size_t)n_jobs * 4, 4}};
    if ((rc = block_upload(block, parts, 11, "the SVR split jobs"))) return rc;
    Staged st;                                        // X goes up once, through the lane's scratch
    if ((rc = stage(st, X, n_dims, n_samples, nullptr, nullptr, 0, {{n_q ? pred_out : nullptr, (size_t)n_q * 8}}))) return rc;
    // solve the batch
    svrfit::SvrDev m = svr_dev(st.feats, parts[0], parts[1], parts[2], parts[3], parts[4], parts[7], n_dims, kernel_type, eps, max_iter);
    SvrFitState s;
    std::vector<int> st_words;
    if ((rc = svr_solve_batch(m, s, tasks, (size_t)n_t, (size_t)n_q, iters_per_launch, st_words, n_launches, use_cache ? cache_bytes : 0,
                              cached)))
        return rc;
    if (job_iterations) HIP_TRY(hipMemcpyAsync(job_iterations, m.iter, (size_t)n_jobs * 4, hipMemcpyDeviceToHost, cs()));
    if (job_n_sv) HIP_TRY(hipMemcpyAsync(job_n_sv, m.n_sv, (size_t)n_jobs * 4, hipMemcpyDeviceToHost, cs()));
    if (train_pred_out) HIP_TRY(hipMemcpyAsync(train_pred_out, m.train_pred, (size_t)n_t * 8, hipMemcpyDeviceToHost, cs()));
    if (job_status) std::copy(st_words.begin(), st_words.end(), job_status);
    // score: the decision value of a job's one pair is sum_t beta_t K(z_t, z) - rho
    if (n_q) {
        const smo::SvcFitDev f = svc_fit_dev(m, m.beta, parts[5], parts[6], parts[8], parts[9], parts[10], nullptr, 1);
        LAUNCH_TRY("SVR scoring", launch::svc_pairs(f, (long long)blocks.size(), s.label, (double *)st.out[0], cs()));
    }
    return finish(st);
}
extern "C" int paa_svr_fit_splits_f64(const double *X, int64_t n_samples, int n_dims, const double *y, int n_jobs, const int64_t *train_off,
                                      const int32_t *train_idx, const int64_t *test_off, const int32_t *test_idx, const double *mean,
                                      const double *std, const double *C, const double *gamma, const double *epsilon, int kernel_type,
                                      double eps, int max_iter, int iters_per_launch, double *pred_out, double *train_pred_out,
                                      int32_t *job_iterations, int32_t *job_status, int32_t *job_n_sv, int32_t *n_launches) {
    return svr_fit_splits_run(X, n_samples, n_dims, y, n_jobs, train_off, train_idx, test_off, test_idx, mean, std, C, gamma, epsilon,
                              kernel_type, eps, max_iter, iters_per_launch, pred_out, train_pred_out, job_iterations, job_status, job_n_sv,
                              n_launches, false, 0, nullptr);
}
extern "C" int paa_svr_fit_splits_cached_f64(const double *X, int64_t n_samples, int n_dims, const double *y, int n_jobs,
                                             const int64_t *train_off, const int32_t *train_idx, const int64_t *test_off,
                                             const int32_t *test_idx, const double *mean, const double *std, const double *C,
                                             const double *gamma, const double *epsilon, int kernel_type, double eps, int max_iter,
                                             int iters_per_launch, double *pred_out, double *train_pred_out, int32_t *job_iterations,
                                             int32_t *job_status, int32_t *job_n_sv, int32_t *n_launches, int64_t cache_bytes,
                                             int32_t *job_cached) {
    return svr_fit_splits_run(X, n_samples, n_dims, y, n_jobs, train_off, train_idx, test_off, test_idx, mean, std, C, gamma, epsilon,
                              kernel_type, eps, max_iter, iters_per_launch, pred_out, train_pred_out, job_iterations, job_status, job_n_sv,
                              n_launches, true, cache_bytes, job_cached);
}
