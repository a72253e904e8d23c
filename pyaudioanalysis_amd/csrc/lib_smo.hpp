// The SVM fits of audioTrainTest.evaluate_classifier (audioTrainTest.py:631-700 with train_svm :132-155) on the device: a batch
// of binary C-SVC dual problems (tasks) over ONE uploaded sample matrix, solved by relaunching smo_kernel until every task has
// stopped, and the split sweep built on it (pair tasks per job, then the one-against-one vote of every test row).
// With resident kernel matrices (DESIGN K23, the *_cached_f64 entry points) the tasks of a GROUP -- one mean / scale / gamma: the pair
// fits and the fold fits of a job -- share one matrix over the group's distinct rows (SmoGroups).  The groups are packed into chunks
// whose matrices fit `cache_bytes` (svr_cache_pack, lib_gramcache.hpp); per chunk: the Gram pass over the groups' row lists, then
// smo_relaunch_some with smo_cached_kernel over the chunk's tasks.  The tasks of a group whose matrix alone exceeds the budget go to
// smo_kernel in the same call.
// Kernels: kernels_smo.hpp and kernels_smocache.hpp (family_smo.hip), kernels_svrcache.hpp (family_svr.hip).
#pragma once

// the limits, for callers and tests: threads per workgroup, groups, rows per task, test rows per scoring workgroup, the default
// iterations per launch, dims
extern "C" int paa_debug_smo_geometry(int32_t *out6) {
    if (!out6) return fail(PAA_ERR_ARG, "null");
    launch::smo_geometry(out6);
    return PAA_OK;
}

// what both entry points ask of the solver's parameters
static int smo_params_check(int n_dims, int kernel_type, double eps, int max_iter, int iters_per_launch) {
    if (n_dims < 1) return fail(PAA_ERR_ARG, "%d feature dimensions", n_dims);
    if (n_dims > smo::kMaxDims) return fail(PAA_ERR_UNSUPPORTED, "%d feature dimensions: at most %d are supported", n_dims, smo::kMaxDims);
    if (kernel_type != 0 && kernel_type != 2) return fail(PAA_ERR_ARG, "kernel type %d: 0 (linear) and 2 (RBF) are supported", kernel_type);
    if (!(eps > 0.0)) return fail(PAA_ERR_ARG, "eps = %g: a positive tolerance is needed", eps);
    if (max_iter < 1) return fail(PAA_ERR_ARG, "max_iter = %d", max_iter);
    if (iters_per_launch < 0) return fail(PAA_ERR_ARG, "iters_per_launch = %d (0: the default, %d)", iters_per_launch, smo::kDefaultItersPerLaunch);
    return PAA_OK;
}
static int smo_task_check(int t, int64_t n, double C, double gamma, int kernel_type) {
    if (n < 1) return fail(PAA_ERR_ARG, "task %d: no rows", t);
    if (n > smo::kMaxRows) return fail(PAA_ERR_UNSUPPORTED, "task %d: %lld rows: at most %d per task are supported", t, (long long)n, smo::kMaxRows);
    if (!(C > 0.0) || !std::isfinite(C)) return fail(PAA_ERR_ARG, "task %d: C = %g", t, C);
    if (kernel_type == 2 && (!(gamma > 0.0) || !std::isfinite(gamma))) return fail(PAA_ERR_ARG, "task %d: gamma = %g", t, gamma);
    return PAA_OK;
}

// The state of a batch on the device, freed on return: alpha | G | QD | alpha_y [rows]; rho | gap [tasks]; iter | status | n_sv |
// live [tasks]
struct SmoState {
    DevBlock block;
    int *live = nullptr;
};
static int smo_state_alloc(SmoState &s, smo::SmoDev &m, size_t rows, size_t n_tasks) {
    const size_t b_rows = up256(rows * 8), b_task8 = up256(n_tasks * 8), b_task4 = up256(n_tasks * 4);
    HIP_TRY(hipMalloc(&s.block.p, 4 * b_rows + 2 * b_task8 + 4 * b_task4));
    char *p = (char *)s.block.p;
    m.alpha = (double *)p;      p += b_rows;
    m.G = (double *)p;          p += b_rows;
    m.QD = (double *)p;         p += b_rows;
    m.alpha_y = (double *)p;    p += b_rows;
    m.rho = (double *)p;        p += b_task8;
    m.gap = (double *)p;        p += b_task8;
    m.iter = (int *)p;          p += b_task4;
    m.status = (int *)p;        p += b_task4;
    m.n_sv = (int *)p;          p += b_task4;
    s.live = (int *)p;
    HIP_TRY(hipMemsetAsync(m.iter, 0, 2 * b_task4, cs()));       // iteration 0, status kFresh
    return PAA_OK;
}

// The relaunch loop of a batch of solver tasks (smo_kernel; svr_smo_kernel and svr_smo_cached_kernel of lib_svrfit.hpp):
// step(n_live, n_max, budget) gives each of the n_live unfinished tasks listed in d_live (n_max: the longest of them) at most `budget`
// iterations (iters_per_launch, 0: the default), the host reads the status words d_status [n_tasks], compacts the unfinished tasks
// and launches again.  smo_relaunch_some runs the tasks of `live` alone and adds its launches to `launches`; status [n_tasks] is the
// caller's and ends as smo::kConverged / kNotConverged for those tasks
template <typename Step>
static int smo_relaunch_some(const std::vector<smo::SmoTask> &tasks, std::vector<int> live, int max_iter, int iters_per_launch, int *d_live,
                             const int *d_status, std::vector<int> &status, long long &launches, Step step) {
    const int budget = iters_per_launch ? iters_per_launch : smo::kDefaultItersPerLaunch;
    const int n_tasks = (int)tasks.size();
    const long long launch_cap = (long long)max_iter / budget + 2;       // every launch advances every live task by `budget`
    long long mine = 0;
    while (!live.empty()) {
        if (mine++ >= launch_cap) return fail(PAA_ERR_HIP, "the solver made no progress in %lld launches", launch_cap);
        int n_max = 0;
        for (int t : live) n_max = std::max(n_max, tasks[t].n);
        HIP_TRY(hipMemcpyAsync(d_live, live.data(), live.size() * 4, hipMemcpyHostToDevice, cs()));
        int rc;
        if ((rc = step((int)live.size(), n_max, budget))) return rc;
        HIP_TRY(hipMemcpyAsync(status.data(), d_status, (size_t)n_tasks * 4, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipStreamSynchronize(cs()));
        size_t kept = 0;
        for (int t : live)
            if (status[t] < smo::kConverged) live[kept++] = t;
        live.resize(kept);
    }
    launches += mine;
    return PAA_OK;
}
template <typename Step>
static int smo_relaunch(const std::vector<smo::SmoTask> &tasks, int max_iter, int iters_per_launch, int *d_live, const int *d_status,
                        std::vector<int> &status, int *n_launches, Step step) {
    const int n_tasks = (int)tasks.size();
    std::vector<int> live(n_tasks);
    for (int t = 0; t < n_tasks; ++t) live[t] = t;
    status.assign(n_tasks, smo::kFresh);
    long long launches = 0;
    int rc;
    if ((rc = smo_relaunch_some(tasks, live, max_iter, iters_per_launch, d_live, d_status, status, launches, step))) return rc;
    if (n_launches) *n_launches = (int)launches;
    return PAA_OK;
}

// Solves a batch: allocates its state into s and m, then runs every task to its stop (smo_relaunch)
static int smo_solve_batch(smo::SmoDev &m, SmoState &s, const std::vector<smo::SmoTask> &tasks, size_t rows, int iters_per_launch,
                           std::vector<int> &status, int *n_launches) {
    int rc;
    if ((rc = smo_state_alloc(s, m, rows, tasks.size()))) return rc;
    return smo_relaunch(tasks, m.max_iter, iters_per_launch, s.live, m.status, status, n_launches, [&](int n_live, int n_max, int budget) {
        LAUNCH_TRY("SMO", launch::smo_step(m, s.live, n_live, n_max, budget, cs()));
        return (int)PAA_OK;
    });
}

// ---- resident kernel matrices (DESIGN K23) ----------------------------------------------------------------------------------------

// The groups of a batch: tasks with equal ids form a group (ids null: every task its own), numbered in order of first appearance.  A
// group's row list is the distinct sample indices of its tasks in order of first appearance over the tasks in task order; `groups`
// holds it as a task of the Gram pass (off into `rows`, n = N, the stat and gamma of the group's first task).  pos [rows of the
// batch]: per task row its place in the group's row list -- a sample listed twice maps to one place
struct SmoGroups {
    std::vector<smo::SmoTask> groups;
    std::vector<int> rows, pos, group_of, first_task;     // group_of [n_tasks]; first_task [n_groups]
};
static void smo_groups_form(SmoGroups &g, const std::vector<smo::SmoTask> &tasks, const int *idx, const int32_t *ids) {
    const size_t nt = tasks.size();
    g.group_of.resize(nt);
    std::vector<std::vector<int>> members;
    std::map<int32_t, int> seen;
    size_t total = 0;
    int top = 0;
    for (size_t t = 0; t < nt; ++t) {
        int gi = (int)members.size();
        if (ids) {
            const auto it = seen.find(ids[t]);
            if (it != seen.end()) gi = it->second;
            else seen[ids[t]] = gi;
        }
        if (gi == (int)members.size()) { members.emplace_back(); g.first_task.push_back((int)t); }
        members[gi].push_back((int)t);
        g.group_of[t] = gi;
        total = std::max(total, (size_t)(tasks[t].off + tasks[t].n));
    }
    for (size_t i = 0; i < total; ++i) top = std::max(top, idx[i]);
    g.pos.assign(total, 0);
    std::vector<int> slot((size_t)top + 1, -1);
    for (size_t gi = 0; gi < members.size(); ++gi) {
        const size_t start = g.rows.size();
        for (int t : members[gi])
            for (long long r = tasks[t].off; r < tasks[t].off + tasks[t].n; ++r) {
                int &at = slot[idx[r]];
                if (at < 0) { at = (int)(g.rows.size() - start); g.rows.push_back(idx[r]); }
                g.pos[r] = at;
            }
        for (size_t k = start; k < g.rows.size(); ++k) slot[g.rows[k]] = -1;
        const smo::SmoTask &F = tasks[g.first_task[gi]];
        g.groups.push_back({(long long)start, (int)(g.rows.size() - start), F.stat, 1.0, F.gamma});
    }
}
// a group's tasks standardise and weigh alike: every byte of their rows of mean / std [..][n_dims] and of their gamma
static int smo_groups_check(const SmoGroups &g, const std::vector<smo::SmoTask> &tasks, const double *mean, const double *std, int n_dims) {
    for (size_t t = 0; t < tasks.size(); ++t) {
        const int f = g.first_task[g.group_of[t]];
        const smo::SmoTask &A = tasks[f], &B = tasks[t];
        const size_t row = (size_t)n_dims * 8;
        const char *what = nullptr;
        if (memcmp(mean + (size_t)A.stat * n_dims, mean + (size_t)B.stat * n_dims, row)) what = "mean";
        else if (memcmp(std + (size_t)A.stat * n_dims, std + (size_t)B.stat * n_dims, row)) what = "scale";
        else if (memcmp(&A.gamma, &B.gamma, 8)) what = "gamma";
        if (what) return fail(PAA_ERR_ARG, "tasks %d and %d are one group and differ in their %s: a group shares one kernel matrix", f, (int)t, what);
    }
    return PAA_OK;
}

// smo_solve_batch from resident matrices under the budget cache_bytes: the groups g of the batch are packed in group order; cached
// [n_groups] (may be null): 1 for a group whose tasks were solved from its matrix
static int smo_solve_batch_cached(smo::SmoDev &m, SmoState &s, const std::vector<smo::SmoTask> &tasks, size_t rows, int iters_per_launch,
                                  std::vector<int> &status, int *n_launches, const SmoGroups &g, int64_t cache_bytes, int32_t *cached) {
    int rc;
    if ((rc = smo_state_alloc(s, m, rows, tasks.size()))) return rc;
    SvrCache c;
    if ((rc = svr_cache_alloc(c, g.groups, m.n_dims, cache_bytes))) return rc;
    const size_t nt = tasks.size(), ng = g.groups.size();
    std::vector<long long> k_off(nt, 0);
    std::vector<int> group_n(nt), members;
    for (size_t t = 0; t < nt; ++t) {
        const int gi = g.group_of[t];
        if (c.chunk_of[gi] >= 0) k_off[t] = c.off[gi];
        else members.push_back((int)t);
        group_n[t] = g.groups[gi].n;
    }
    for (size_t gi = 0; cached && gi < ng; ++gi) cached[gi] = c.chunk_of[gi] >= 0;
    DevBlock block;
    BlockPart parts[] = {{g.groups.data(), ng * sizeof(smo::SmoTask), 8}, {k_off.data(), nt * 8, 8}, {g.rows.data(), g.rows.size() * 4, 4},
                         {g.pos.data(), g.pos.size() * 4, 4}, {group_n.data(), nt * 4, 4}};
    if (c.n_chunks && (rc = block_upload(block, parts, 5, "the SMO groups"))) return rc;
    svrfit::SvrDev gm{};                              // the Gram pass's view: a group's row list is its task
    gm.X = m.X;
    gm.idx = (const int *)parts[2].dev;
    gm.tasks = (const smo::SmoTask *)parts[0].dev;
    gm.mean = m.mean;
    gm.scale = m.scale;
    gm.n_dims = m.n_dims;
    gm.rbf = m.rbf;
    const smo::SmoCacheDev cd{c.dev.K, (const long long *)parts[1].dev, (const int *)parts[4].dev, (const int *)parts[3].dev};
    status.assign(nt, smo::kFresh);
    long long launches = 0;
    const auto plain = [&](int n_live, int n_max, int budget) {
        LAUNCH_TRY("SMO", launch::smo_step(m, s.live, n_live, n_max, budget, cs()));
        return (int)PAA_OK;
    };
    const auto from_matrix = [&](int n_live, int, int budget) {
        LAUNCH_TRY("cached SMO", launch::smo_cached_step(m, cd, s.live, n_live, budget, cs()));
        return (int)PAA_OK;
    };
    if (!members.empty() && (rc = smo_relaunch_some(tasks, members, m.max_iter, iters_per_launch, s.live, m.status, status, launches, plain)))
        return rc;
    std::vector<int> chunk_groups;
    for (int ch = 0; ch < c.n_chunks; ++ch) {
        if ((rc = svr_cache_fill(c, gm, g.groups, ch, chunk_groups))) return rc;
        members.clear();
        for (size_t t = 0; t < nt; ++t)
            if (c.chunk_of[g.group_of[t]] == ch) members.push_back((int)t);
        if ((rc = smo_relaunch_some(tasks, members, m.max_iter, iters_per_launch, s.live, m.status, status, launches, from_matrix))) return rc;
    }
    if (n_launches) *n_launches = (int)launches;
    return PAA_OK;
}

// The layout alone, on the host, for tests: the groups of the task row lists task_off / task_idx under the ids `group` (null: every
// task its own) and the chunk of every group under cache_bytes; see paa_hip.h
extern "C" int paa_debug_smo_cache_layout(int n_tasks, const int64_t *task_off, const int32_t *task_idx, const int32_t *group,
                                          int64_t cache_bytes, int32_t *n_groups, int32_t *group_of, int64_t *group_off,
                                          int32_t *group_rows, int32_t *pos, int32_t *group_chunk) {
    if (!task_off || !task_idx || !n_groups || !group_of || !group_off || !group_rows || !pos || !group_chunk) return fail(PAA_ERR_ARG, "null argument");
    if (n_tasks < 1) return fail(PAA_ERR_ARG, "no tasks");
    int rc;
    if ((rc = sweep_offsets_check(task_off, n_tasks, "task"))) return rc;
    if ((rc = svr_cache_args_check(cache_bytes))) return rc;
    std::vector<smo::SmoTask> tasks(n_tasks);
    for (int t = 0; t < n_tasks; ++t) {
        const int64_t n = task_off[t + 1] - task_off[t];
        if (n < 1 || n > 0x7fffffffLL) return fail(PAA_ERR_ARG, "task %d: %lld rows", t, (long long)n);
        tasks[t] = {(long long)task_off[t], (int)n, t, 1.0, 1.0};
    }
    for (int64_t i = 0; i < task_off[n_tasks]; ++i)
        if (task_idx[i] < 0) return fail(PAA_ERR_ARG, "row index %d", task_idx[i]);
    SmoGroups g;
    smo_groups_form(g, tasks, task_idx, group);
    std::vector<int> chunk_of;
    svr_cache_pack(g.groups, cache_bytes, chunk_of);
    *n_groups = (int32_t)g.groups.size();
    std::copy(g.group_of.begin(), g.group_of.end(), group_of);
    std::copy(g.rows.begin(), g.rows.end(), group_rows);
    std::copy(g.pos.begin(), g.pos.end(), pos);
    std::copy(chunk_of.begin(), chunk_of.end(), group_chunk);
    for (size_t gi = 0; gi < g.groups.size(); ++gi) group_off[gi] = g.groups[gi].off;
    group_off[g.groups.size()] = (int64_t)g.rows.size();
    return PAA_OK;
}

// the solver's view of an uploaded batch: the staged matrix, the uploaded tasks | mean | scale | idx | sign and the parameters
static smo::SmoDev smo_dev(const double *X, const BlockPart &tasks, const BlockPart &mean, const BlockPart &scale, const BlockPart &idx,
                           const BlockPart &sign, int n_dims, int kernel_type, double eps, int max_iter) {
    smo::SmoDev m{};
    m.X = X;
    m.tasks = (const smo::SmoTask *)tasks.dev;
    m.mean = (const double *)mean.dev;
    m.scale = (const double *)scale.dev;
    m.idx = (const int *)idx.dev;
    m.sign = (const signed char *)sign.dev;
    m.n_dims = n_dims;
    m.rbf = kernel_type == 2;
    m.max_iter = max_iter;
    m.eps = eps;
    return m;
}

// the scoring kernel's view of the fitted tasks of a solver batch m (smo::SmoDev, svrfit::SvrDev): the uploaded test_off | blocks |
// test_idx | job_task | job_k, the device array job_stat (null: a job standardises with its own row) and the tasks' coefficients
template <typename Dev>
static smo::SvcFitDev svc_fit_dev(const Dev &m, const double *alpha_y, const BlockPart &test_off, const BlockPart &blocks,
                                  const BlockPart &test_idx, const BlockPart &job_task, const BlockPart &job_k, const int *job_stat,
                                  int max_pairs) {
    smo::SvcFitDev f{};
    f.X = m.X;
    f.test_off = (const long long *)test_off.dev;
    f.blocks = (const knn::SplitBlock *)blocks.dev;
    f.test_idx = (const int *)test_idx.dev;
    f.job_task = (const int *)job_task.dev;
    f.job_k = (const int *)job_k.dev;
    f.job_stat = job_stat;
    f.mean = m.mean;
    f.scale = m.scale;
    f.tasks = m.tasks;
    f.idx = m.idx;
    f.alpha_y = alpha_y;
    f.rho = m.rho;
    f.n_dims = m.n_dims;
    f.rbf = m.rbf;
    f.max_pairs = max_pairs;
    return f;
}

// The solver alone (libsvm's Solver::Solve for C-SVC, svm.cpp, as svm_train_one runs it under SVC.fit): see paa_hip.h
// (use_cache false: paa_smo_tasks_f64; true: paa_smo_tasks_cached_f64 with its groups, budget and flags)
static int smo_tasks_run(const double *X, int64_t n_samples, int n_dims, int n_tasks, const int64_t *task_off, const int32_t *task_idx,
                         const int8_t *task_sign, const double *mean, const double *std, const double *C, const double *gamma,
                         int kernel_type, double eps, int max_iter, int iters_per_launch, double *alpha_y, double *rho,
                         int32_t *iterations, double *gap, int32_t *status, int32_t *n_launches, bool use_cache, const int32_t *group,
                         int64_t cache_bytes, int32_t *cached) {
    if (!X || !task_off || !task_idx || !task_sign || !mean || !std || !C || !gamma || !alpha_y || !rho || !iterations || !gap || !status ||
        (use_cache && !cached))
        return fail(PAA_ERR_ARG, "null argument");
    int rc;
    if ((rc = sweep_samples_check(n_samples))) return rc;
    if ((rc = smo_params_check(n_dims, kernel_type, eps, max_iter, iters_per_launch))) return rc;
    if (n_tasks < 1) return fail(PAA_ERR_ARG, "no tasks");
    if ((rc = sweep_offsets_check(task_off, n_tasks, "task"))) return rc;
    const int64_t rows = task_off[n_tasks];
    std::vector<smo::SmoTask> tasks(n_tasks);
    for (int t = 0; t < n_tasks; ++t) {
        if ((rc = smo_task_check(t, task_off[t + 1] - task_off[t], C[t], gamma[t], kernel_type))) return rc;
        tasks[t] = {(long long)task_off[t], (int)(task_off[t + 1] - task_off[t]), t, C[t], gamma[t]};
    }
    if ((rc = sweep_index_check(task_idx, rows, n_samples, "row"))) return rc;
    for (int64_t i = 0; i < rows; ++i)
        if (task_sign[i] != 1 && task_sign[i] != -1) return fail(PAA_ERR_ARG, "sign %d of row %lld: +1 or -1", (int)task_sign[i], (long long)i);
    SmoGroups g;
    if (use_cache) {
        if ((rc = svr_cache_args_check(cache_bytes))) return rc;
        smo_groups_form(g, tasks, task_idx, group);
        if ((rc = smo_groups_check(g, tasks, mean, std, n_dims))) return rc;
    }
    if ((rc = ensure_init())) return rc;
    const size_t sb = (size_t)n_tasks * n_dims * 8;
    DevBlock block;
    BlockPart parts[] = {{tasks.data(), tasks.size() * sizeof(smo::SmoTask), 8}, {mean, sb, 8}, {std, sb, 8},
                         {task_idx, (size_t)rows * 4, 4}, {task_sign, (size_t)rows, 1}};
    if ((rc = block_upload(block, parts, 5, "the SMO tasks"))) return rc;
    Staged st;                                        // X goes up once, through the lane's scratch
    if ((rc = stage(st, X, n_dims, n_samples, nullptr, nullptr, 0, {}))) return rc;
    smo::SmoDev m = smo_dev(st.feats, parts[0], parts[1], parts[2], parts[3], parts[4], n_dims, kernel_type, eps, max_iter);
    SmoState s;
    std::vector<int> st_words;
    if (use_cache) {
        std::vector<int32_t> group_cached(g.groups.size());
        if ((rc = smo_solve_batch_cached(m, s, tasks, (size_t)rows, iters_per_launch, st_words, n_launches, g, cache_bytes, group_cached.data())))
            return rc;
        for (int t = 0; t < n_tasks; ++t) cached[t] = group_cached[g.group_of[t]];
    } else if ((rc = smo_solve_batch(m, s, tasks, (size_t)rows, iters_per_launch, st_words, n_launches))) {
        return rc;
    }
    HIP_TRY(hipMemcpyAsync(alpha_y, m.alpha_y, (size_t)rows * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(rho, m.rho, (size_t)n_tasks * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(gap, m.gap, (size_t)n_tasks * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(iterations, m.iter, (size_t)n_tasks * 4, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    std::copy(st_words.begin(), st_words.end(), status);
    return PAA_OK;
}
extern "C" int paa_smo_tasks_f64(const double *X, int64_t n_samples, int n_dims, int n_tasks, const int64_t *task_off,
                                 const int32_t *task_idx, const int8_t *task_sign, const double *mean, const double *std,
                                 const double *C, const double *gamma, int kernel_type, double eps, int max_iter,
                                 int iters_per_launch, double *alpha_y, double *rho, int32_t *iterations, double *gap,
                                 int32_t *status, int32_t *n_launches) {
    return smo_tasks_run(X, n_samples, n_dims, n_tasks, task_off, task_idx, task_sign, mean, std, C, gamma, kernel_type, eps, max_iter,
                         iters_per_launch, alpha_y, rho, iterations, gap, status, n_launches, false, nullptr, 0, nullptr);
}
extern "C" int paa_smo_tasks_cached_f64(const double *X, int64_t n_samples, int n_dims, int n_tasks, const int64_t *task_off,
                                        const int32_t *task_idx, const int8_t *task_sign, const double *mean, const double *std,
                                        const double *C, const double *gamma, int kernel_type, double eps, int max_iter,
                                        int iters_per_launch, double *alpha_y, double *rho, int32_t *iterations, double *gap,
                                        int32_t *status, int32_t *n_launches, const int32_t *group, int64_t cache_bytes,
                                        int32_t *cached) {
    return smo_tasks_run(X, n_samples, n_dims, n_tasks, task_off, task_idx, task_sign, mean, std, C, gamma, kernel_type, eps, max_iter,
                         iters_per_launch, alpha_y, rho, iterations, gap, status, n_launches, true, group, cache_bytes, cached);
}

// the ids that make every job of a sweep one group: a task's stat is its job
static std::vector<int32_t> smo_job_ids(const std::vector<smo::SmoTask> &tasks) {
    std::vector<int32_t> ids(tasks.size());
    for (size_t t = 0; t < tasks.size(); ++t) ids[t] = tasks[t].stat;
    return ids;
}

// The pair tasks of a split sweep: per job the classes present in its training list, ascending; per pair (a, b), a < b, one task
// over the rows of a in train-list order (sign +1), then those of b (sign -1)
struct PairTasks {
    std::vector<smo::SmoTask> tasks;
    std::vector<int> idx, job_task, job_k, job_class;     // job_task [n_jobs + 1]; job_class: every job's classes, job after job
    std::vector<signed char> sign;
    std::vector<size_t> job_class_off;                    // [n_jobs + 1] into job_class
    int pairs_max = 0;
};
static int svc_pair_tasks(PairTasks &p, const int32_t *labels, int n_jobs, const int64_t *train_off, const int32_t *train_idx,
                          const double *C, const double *gamma, int kernel_type) {
    p.job_task.assign(n_jobs + 1, 0);
    p.job_k.assign(n_jobs, 0);
    p.job_class_off.assign(n_jobs + 1, 0);
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *tr = train_idx + train_off[j];
        const int64_t n_train = train_off[j + 1] - train_off[j];
        std::vector<int> classes;
        for (int64_t i = 0; i < n_train; ++i) classes.push_back(labels[tr[i]]);
        std::sort(classes.begin(), classes.end());
        classes.erase(std::unique(classes.begin(), classes.end()), classes.end());
        const int k = (int)classes.size();
        if (k < 2) return fail(PAA_ERR_ARG, "job %d: %d class(es) in its training list: an SVM needs two", j, k);
        if (k > smo::kMaxClasses) return fail(PAA_ERR_UNSUPPORTED, "job %d: %d classes: at most %d are supported", j, k, smo::kMaxClasses);
        std::vector<std::vector<int>> rows(k);
        for (int64_t i = 0; i < n_train; ++i)
            rows[std::lower_bound(classes.begin(), classes.end(), labels[tr[i]]) - classes.begin()].push_back(tr[i]);
        for (int a = 0; a < k; ++a)
            for (int b = a + 1; b < k; ++b) {
                const int64_t n = (int64_t)rows[a].size() + (int64_t)rows[b].size();
                int rc;
                if ((rc = smo_task_check((int)p.tasks.size(), n, C[j], gamma[j], kernel_type))) return rc;
                p.tasks.push_back({(long long)p.idx.size(), (int)n, j, C[j], gamma[j]});
                p.idx.insert(p.idx.end(), rows[a].begin(), rows[a].end());
                p.idx.insert(p.idx.end(), rows[b].begin(), rows[b].end());
                p.sign.insert(p.sign.end(), rows[a].size(), (signed char)1);
                p.sign.insert(p.sign.end(), rows[b].size(), (signed char)-1);
            }
        if (p.tasks.size() > 0x3fffffffULL) return fail(PAA_ERR_UNSUPPORTED, "too many tasks");
        p.job_k[j] = k;
        p.job_task[j + 1] = (int)p.tasks.size();
        p.job_class.insert(p.job_class.end(), classes.begin(), classes.end());
        p.job_class_off[j + 1] = p.job_class.size();
        p.pairs_max = std::max(p.pairs_max, k * (k - 1) / 2);
    }
    return PAA_OK;
}

// The SVM half of audioTrainTest.evaluate_classifier (audioTrainTest.py:631-700): every split a job, every pair of the classes
// present in its training list a task; see paa_hip.h
// (use_cache false: paa_svc_fit_splits_f64; true: paa_svc_fit_splits_cached_f64 with its budget and flags: a job is a group)
static int svc_fit_splits_run(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs, const int64_t *train_off,
                              const int32_t *train_idx, const int64_t *test_off, const int32_t *test_idx, const double *mean,
                              const double *std, const double *C, const double *gamma, int kernel_type, double eps, int max_iter,
                              int iters_per_launch, int32_t *label_out, double *dec_out, int max_pairs, int n_tasks,
                              int32_t *task_iterations, int32_t *task_status, int32_t *task_n_sv, int32_t *n_launches, bool use_cache,
                              int64_t cache_bytes, int32_t *job_cached) {
    // check
    if (!X || !labels || !train_off || !train_idx || !test_off || !test_idx || !mean || !std || !C || !gamma || !label_out ||
        (use_cache && !job_cached))
        return fail(PAA_ERR_ARG, "null argument");
    int rc;
    if ((rc = sweep_samples_check(n_samples))) return rc;
    if ((rc = smo_params_check(n_dims, kernel_type, eps, max_iter, iters_per_launch))) return rc;
    if ((rc = sweep_jobs_check(n_jobs, train_off, test_off))) return rc;
    const int64_t n_q = test_off[n_jobs], n_t = train_off[n_jobs];
    if ((rc = sweep_index_check(train_idx, n_t, n_samples, "train"))) return rc;
    for (int64_t i = 0; i < n_t; ++i)
        if (labels[train_idx[i]] < 0) return fail(PAA_ERR_ARG, "training sample %d has the label %d: class indices are >= 0", train_idx[i], labels[train_idx[i]]);
    if ((rc = sweep_index_check(test_idx, n_q, n_samples, "test"))) return rc;
    // the pair tasks
    PairTasks p;
    if ((rc = svc_pair_tasks(p, labels, n_jobs, train_off, train_idx, C, gamma, kernel_type))) return rc;
    if (dec_out && max_pairs < p.pairs_max) return fail(PAA_ERR_ARG, "max_pairs = %d, a job has %d pairs", max_pairs, p.pairs_max);
    if ((task_iterations || task_status || task_n_sv) && n_tasks != (int)p.tasks.size())
        return fail(PAA_ERR_ARG, "n_tasks = %d, the jobs make %d tasks", n_tasks, (int)p.tasks.size());
    if (!dec_out) max_pairs = p.pairs_max;
    if (use_cache && (rc = svr_cache_args_check(cache_bytes))) return rc;
    if ((rc = ensure_init())) return rc;
    // upload
    const std::vector<knn::SplitBlock> blocks = sweep_blocks(test_off, n_jobs, smo::kQueriesPerBlock);
    const size_t sb = (size_t)n_jobs * n_dims * 8, rows = p.idx.size(), nt = p.tasks.size();
    const knn::SplitBlock none{0, 0};
    DevBlock block;
    BlockPart parts[] = {{p.tasks.data(), nt * sizeof(smo::SmoTask), 8},
                         {mean, sb, 8},
                         {std, sb, 8},
                         {test_off, (size_t)(n_jobs + 1) * 8, 8},
                         {blocks.empty() ? &none : blocks.data(), std::max<size_t>(blocks.size(), 1) * sizeof(knn::SplitBlock), 8},
                         {p.idx.data(), rows * 4, 4},
                         {n_q ? test_idx : p.idx.data(), (size_t)std::max<int64_t>(n_q, 1) * 4, 4},
                         {p.job_task.data(), (size_t)(n_jobs + 1) * 4, 4},
                         {p.job_k.data(), (size_t)n_jobs * 4, 4},
                         {p.sign.data(), rows, 1}};
    if ((rc = block_upload(block, parts, 10, "the SVM split jobs"))) return rc;
    Staged st;                                        // X goes up once, through the lane's scratch
    if ((rc = stage(st, X, n_dims, n_samples, nullptr, nullptr, 0,
                    {{n_q ? label_out : nullptr, (size_t)n_q * 4}, {n_q ? dec_out : nullptr, (size_t)n_q * max_pairs * 8}})))
        return rc;
    // solve the batch
    smo::SmoDev m = smo_dev(st.feats, parts[0], parts[1], parts[2], parts[5], parts[9], n_dims, kernel_type, eps, max_iter);
    SmoState s;
    std::vector<int> st_words;
    if (use_cache) {                                  // every job has a task, in job order: group j is job j
        SmoGroups g;
        smo_groups_form(g, p.tasks, p.idx.data(), smo_job_ids(p.tasks).data());
        if ((rc = smo_solve_batch_cached(m, s, p.tasks, rows, iters_per_launch, st_words, n_launches, g, cache_bytes, job_cached))) return rc;
    } else if ((rc = smo_solve_batch(m, s, p.tasks, rows, iters_per_launch, st_words, n_launches))) {
        return rc;
    }
    if (task_iterations) HIP_TRY(hipMemcpyAsync(task_iterations, m.iter, nt * 4, hipMemcpyDeviceToHost, cs()));
    if (task_n_sv) HIP_TRY(hipMemcpyAsync(task_n_sv, m.n_sv, nt * 4, hipMemcpyDeviceToHost, cs()));
    if (task_status) std::copy(st_words.begin(), st_words.end(), task_status);
    // vote
    if (n_q) {
        const smo::SvcFitDev f = svc_fit_dev(m, m.alpha_y, parts[3], parts[4], parts[6], parts[7], parts[8], nullptr, max_pairs);
        if (st.out[1]) HIP_TRY(hipMemsetAsync(st.out[1], 0, (size_t)n_q * max_pairs * 8, cs()));     // zeros past a job's pairs
        LAUNCH_TRY("SVM vote", launch::svc_pairs(f, (long long)blocks.size(), (int32_t *)st.out[0], (double *)st.out[1], cs()));
    }
    if ((rc = finish(st))) return rc;
    // a label is the position among the job's classes: back to class indices
    for (int j = 0; j < n_jobs; ++j)
        for (int64_t q = test_off[j]; q < test_off[j + 1]; ++q) label_out[q] = p.job_class[p.job_class_off[j] + label_out[q]];
    return PAA_OK;
}
extern "C" int paa_svc_fit_splits_f64(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs,
                                      const int64_t *train_off, const int32_t *train_idx, const int64_t *test_off,
                                      const int32_t *test_idx, const double *mean, const double *std, const double *C,
                                      const double *gamma, int kernel_type, double eps, int max_iter, int iters_per_launch,
                                      int32_t *label_out, double *dec_out, int max_pairs, int n_tasks, int32_t *task_iterations,
                                      int32_t *task_status, int32_t *task_n_sv, int32_t *n_launches) {
    return svc_fit_splits_run(X, n_samples, n_dims, labels, n_jobs, train_off, train_idx, test_off, test_idx, mean, std, C, gamma,
                              kernel_type, eps, max_iter, iters_per_launch, label_out, dec_out, max_pairs, n_tasks, task_iterations,
                              task_status, task_n_sv, n_launches, false, 0, nullptr);
}
extern "C" int paa_svc_fit_splits_cached_f64(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs,
                                             const int64_t *train_off, const int32_t *train_idx, const int64_t *test_off,
                                             const int32_t *test_idx, const double *mean, const double *std, const double *C,
                                             const double *gamma, int kernel_type, double eps, int max_iter, int iters_per_launch,
                                             int32_t *label_out, double *dec_out, int max_pairs, int n_tasks,
                                             int32_t *task_iterations, int32_t *task_status, int32_t *task_n_sv, int32_t *n_launches,
                                             int64_t cache_bytes, int32_t *job_cached) {
    return svc_fit_splits_run(X, n_samples, n_dims, labels, n_jobs, train_off, train_idx, test_off, test_idx, mean, std, C, gamma,
                              kernel_type, eps, max_iter, iters_per_launch, label_out, dec_out, max_pairs, n_tasks, task_iterations,
                              task_status, task_n_sv, n_launches, true, cache_bytes, job_cached);
}

// ---- probability=True's second half (svm.cpp: svm_binary_svc_probability, sigmoid_train) ----------------------------------------

// Fits the n problems dec / sign / off (device arrays) with one launch of platt_sigmoid_kernel; the outputs go to host arrays
static int platt_run(const double *d_dec, const signed char *d_sign, const long long *d_off, int n, int l_max, double *A, double *B,
                     int32_t *iterations, int32_t *stop) {
    const size_t b8 = up256((size_t)n * 8), b4 = up256((size_t)n * 4);
    DevBlock out;
    HIP_TRY(hipMalloc(&out.p, 2 * b8 + 2 * b4));
    platt::PlattDev p{};
    p.dec = d_dec;
    p.sign = d_sign;
    p.off = d_off;
    p.A = (double *)out.p;
    p.B = (double *)((char *)out.p + b8);
    p.iter = (int *)((char *)out.p + 2 * b8);
    p.stop = (int *)((char *)out.p + 2 * b8 + b4);
    LAUNCH_TRY("sigmoid fit", launch::platt_sigmoid(p, n, l_max, cs()));
    HIP_TRY(hipMemcpyAsync(A, p.A, (size_t)n * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(B, p.B, (size_t)n * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(iterations, p.iter, (size_t)n * 4, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(stop, p.stop, (size_t)n * 4, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}

// the problems of a sigmoid launch: offsets from 0, 1 .. platt::kMaxRows values each; l_max: the longest
static int platt_offsets_check(const int64_t *off, int n, int *l_max) {
    int rc;
    if ((rc = sweep_offsets_check(off, n, "problem"))) return rc;
    *l_max = 0;
    for (int p = 0; p < n; ++p) {
        const int64_t l = off[p + 1] - off[p];
        if (l < 1) return fail(PAA_ERR_ARG, "problem %d: no values", p);
        if (l > platt::kMaxRows) return fail(PAA_ERR_UNSUPPORTED, "problem %d: %lld values: at most %d per problem are supported", p, (long long)l, platt::kMaxRows);
        *l_max = std::max(*l_max, (int)l);
    }
    return PAA_OK;
}

// The sigmoid fit alone: see paa_hip.h
extern "C" int paa_platt_sigmoid_f64(const double *dec, const int8_t *sign, int n_problems, const int64_t *prob_off, double *A, double *B,
                                     int32_t *iterations, int32_t *stop) {
    if (!dec || !sign || !prob_off || !A || !B || !iterations || !stop) return fail(PAA_ERR_ARG, "null argument");
    if (n_problems < 1) return fail(PAA_ERR_ARG, "no problems");
    int rc, l_max;
    if ((rc = platt_offsets_check(prob_off, n_problems, &l_max))) return rc;
    const int64_t total = prob_off[n_problems];
    for (int64_t i = 0; i < total; ++i)
        if (sign[i] != 1 && sign[i] != -1) return fail(PAA_ERR_ARG, "sign %d of value %lld: +1 or -1", (int)sign[i], (long long)i);
    if ((rc = ensure_init())) return rc;
    LaneGuard lane;       // own stream for this call (see Lane)
    DevBlock block;
    BlockPart parts[] = {{dec, (size_t)total * 8, 8}, {prob_off, (size_t)(n_problems + 1) * 8, 8}, {sign, (size_t)total, 1}};
    if ((rc = block_upload(block, parts, 3, "the sigmoid problems"))) return rc;
    return platt_run((const double *)parts[0].dev, (const signed char *)parts[2].dev, (const long long *)parts[1].dev, n_problems, l_max,
                     A, B, iterations, stop);
}

// libsvm's bounded draw (scikit-learn's newrand.h: Lemire's method with rejection over std::mt19937)
static uint32_t platt_bounded(std::mt19937 &gen, uint32_t range) {
    uint64_t m = (uint64_t)(uint32_t)gen() * range;
    uint32_t low = (uint32_t)m;
    if (low < range) {
        const uint32_t t = (uint32_t)(0u - range) % range;
        while (low < t) {
            m = (uint64_t)(uint32_t)gen() * range;
            low = (uint32_t)m;
        }
    }
    return (uint32_t)(m >> 32);
}

// The folds of svm_binary_svc_probability over the pair tasks p (svc_pair_tasks): per pair the permutation of its rows from the
// job's seed; per fold with both classes in its training part one task appended to p (rows in permutation order, grouped by
// class, the class seen first put first) and, when it holds rows out, one scoring job.  cv [rows of the pairs] receives the
// constants of the folds that make no task; where [Q] is the place in cv of every scored row, fold_task [pairs][5] the task of a
// fold (-1: none)
struct PlattFolds {
    std::vector<int64_t> test_off{0};     // [n_score + 1]
    std::vector<int> test_idx, job_task, job_stat;      // held-out sample rows; per scoring job its task and its job
    std::vector<int64_t> where;
    std::vector<int> fold_task;
};
static int platt_folds(PlattFolds &f, PairTasks &p, const int64_t *seed, std::vector<double> &cv, int kernel_type) {
    const int n_pairs = (int)p.tasks.size();
    f.fold_task.assign((size_t)n_pairs * 5, -1);
    std::vector<int> perm, first, second;
    for (int t = 0; t < n_pairs; ++t) {
        const smo::SmoTask T = p.tasks[t];
        const int l = T.n;
        std::mt19937 gen((uint32_t)seed[T.stat]);
        perm.resize(l);
        for (int i = 0; i < l; ++i) perm[i] = i;
        for (int i = 0; i < l; ++i) std::swap(perm[i], perm[i + (int)platt_bounded(gen, (uint32_t)(l - i))]);
        for (int fold = 0; fold < 5; ++fold) {
            const int begin = (int)((int64_t)fold * l / 5), end = (int)((int64_t)(fold + 1) * l / 5);
            first.clear();
            second.clear();
            int lead = 0;                                 // the sign of the class seen first
            for (int k = 0; k < l; ++k) {
                if (k >= begin && k < end) continue;
                const int s = p.sign[T.off + perm[k]];
                if (!lead) lead = s;
                (s == lead ? first : second).push_back(perm[k]);
            }
            if (second.empty()) {                         // one class or none: no fit
                for (int k = begin; k < end; ++k) cv[T.off + perm[k]] = (double)lead;
                continue;
            }
            int rc;
            const int64_t n = (int64_t)first.size() + (int64_t)second.size();
            if ((rc = smo_task_check((int)p.tasks.size(), n, T.C, T.gamma, kernel_type))) return rc;
            f.fold_task[(size_t)t * 5 + fold] = (int)p.tasks.size();
            p.tasks.push_back({(long long)p.idx.size(), (int)n, T.stat, T.C, T.gamma});
            for (const std::vector<int> *rows : {&first, &second})
                for (int r : *rows) {
                    const int sample = p.idx[T.off + r];
                    const signed char sg = p.sign[T.off + r];
                    p.idx.push_back(sample);
                    p.sign.push_back(sg);
                }
            if (end > begin) {
                f.job_task.push_back(f.fold_task[(size_t)t * 5 + fold]);
                f.job_stat.push_back(T.stat);
                for (int k = begin; k < end; ++k) {
                    f.test_idx.push_back(p.idx[T.off + perm[k]]);
                    f.where.push_back(T.off + perm[k]);
                }
                f.test_off.push_back((int64_t)f.test_idx.size());
            }
        }
    }
    return PAA_OK;
}

// What svc_fit_proba_resident gives back: host arrays, paa_svc_fit_proba_f64's outputs of the same names (cv_dec and n_launches may
// be null) and paa_svc_fit_proba_cached_f64's job_cached (null: no resident matrices; else with the budget cache_bytes)
struct ProbaFitOut {
    double *alpha_y, *rho, *prob_a, *prob_b;
    int32_t *n_sv, *task_iterations, *task_status, *sig_iterations, *sig_stop;
    double *cv_dec;
    int32_t *n_launches;
    int32_t *job_cached = nullptr;
    int64_t cache_bytes = 0;
};

// The fits of SVC(probability=True) over a sample matrix that is already RESIDENT (d_X [..][n_dims], with d_mean / d_scale
// [n_jobs][n_dims] on the device too): p holds the pair tasks of the jobs (svc_pair_tasks) and receives the folds; the full fits
// and the fold fits are one solver batch, svc_pairs_kernel scores every fold's held-out rows, platt_sigmoid_kernel fits every
// pair.  With o.job_cached the full fits and the fold fits of a job are one group and read one resident matrix
// (smo_solve_batch_cached).  Runs on the caller's stream (cs()) and has finished when it returns
static int svc_fit_proba_resident(const double *d_X, const double *d_mean, const double *d_scale, int n_dims, PairTasks &p,
                                  const int64_t *seed, int kernel_type, double eps, int max_iter, int iters_per_launch,
                                  const ProbaFitOut &o) {
    int rc;
    const size_t np = p.tasks.size(), rows_full = p.idx.size();
    std::vector<int64_t> prob_off(np + 1, 0);
    int l_max = 0;
    for (size_t t = 0; t < np; ++t) {
        prob_off[t + 1] = prob_off[t] + p.tasks[t].n;
        l_max = std::max(l_max, p.tasks[t].n);
    }
    std::vector<double> cv(rows_full, 0.0);
    PlattFolds f;
    if ((rc = platt_folds(f, p, seed, cv, kernel_type))) return rc;
    if (p.tasks.size() > 0x3fffffffULL || f.test_idx.size() > (size_t)kSweepMaxQ) return fail(PAA_ERR_UNSUPPORTED, "too many tasks");
    // upload: a fold with held-out rows is a scoring job of one pair, standardised as its job
    const int n_score = (int)f.job_task.size();
    const int64_t n_q = f.test_off[n_score];
    const std::vector<knn::SplitBlock> blocks = sweep_blocks(f.test_off.data(), n_score, smo::kQueriesPerBlock);
    std::vector<int> job_k((size_t)std::max(n_score, 1), 2);
    f.job_task.push_back((int)p.tasks.size());
    if (f.job_stat.empty()) f.job_stat.push_back(0);
    const size_t rows = p.idx.size(), nt = p.tasks.size();
    const knn::SplitBlock none{0, 0};
    DevBlock block;
    BlockPart parts[] = {{p.tasks.data(), nt * sizeof(smo::SmoTask), 8},
                         {f.test_off.data(), (size_t)(n_score + 1) * 8, 8},
                         {prob_off.data(), (np + 1) * 8, 8},
                         {blocks.empty() ? &none : blocks.data(), std::max<size_t>(blocks.size(), 1) * sizeof(knn::SplitBlock), 8},
                         {nullptr, (size_t)std::max<int64_t>(n_q, 1) * 8, 8},           // the held-out decision values
                         {p.idx.data(), rows * 4, 4},
                         {n_q ? f.test_idx.data() : p.idx.data(), (size_t)std::max<int64_t>(n_q, 1) * 4, 4},
                         {f.job_task.data(), (size_t)(n_score + 1) * 4, 4},
                         {job_k.data(), job_k.size() * 4, 4},
                         {f.job_stat.data(), f.job_stat.size() * 4, 4},
                         {nullptr, (size_t)std::max<int64_t>(n_q, 1) * 4, 4},           // their labels (not read)
                         {p.sign.data(), rows, 1}};
    if ((rc = block_upload(block, parts, 12, "the probabilistic SVM jobs"))) return rc;
    std::vector<double> q_dec((size_t)n_q);
    // solve the batch
    smo::SmoDev m{};
    m.X = d_X;
    m.tasks = (const smo::SmoTask *)parts[0].dev;
    m.mean = d_mean;
    m.scale = d_scale;
    m.idx = (const int *)parts[5].dev;
    m.sign = (const signed char *)parts[11].dev;
    m.n_dims = n_dims;
    m.rbf = kernel_type == 2;
    m.max_iter = max_iter;
    m.eps = eps;
    SmoState s;
    std::vector<int> st_words;
    if (o.job_cached) {                               // every job has a pair task, in job order: group j is job j
        SmoGroups g;
        smo_groups_form(g, p.tasks, p.idx.data(), smo_job_ids(p.tasks).data());
        if ((rc = smo_solve_batch_cached(m, s, p.tasks, rows, iters_per_launch, st_words, o.n_launches, g, o.cache_bytes, o.job_cached)))
            return rc;
    } else if ((rc = smo_solve_batch(m, s, p.tasks, rows, iters_per_launch, st_words, o.n_launches))) {
        return rc;
    }
    std::vector<int32_t> iters(nt);
    HIP_TRY(hipMemcpyAsync(iters.data(), m.iter, nt * 4, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(o.alpha_y, m.alpha_y, rows_full * 8, hipMemcpyDeviceToHost, cs()));      // the full fits come first
    HIP_TRY(hipMemcpyAsync(o.rho, m.rho, np * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(o.n_sv, m.n_sv, np * 4, hipMemcpyDeviceToHost, cs()));
    // score the held-out rows of every fold
    if (n_q) {
        const smo::SvcFitDev v = svc_fit_dev(m, m.alpha_y, parts[1], parts[3], parts[6], parts[7], parts[8], (const int *)parts[9].dev, 1);
        LAUNCH_TRY("fold scoring", launch::svc_pairs(v, (long long)blocks.size(), (int32_t *)parts[10].dev, (double *)parts[4].dev, cs()));
        HIP_TRY(hipMemcpyAsync(q_dec.data(), parts[4].dev, (size_t)n_q * 8, hipMemcpyDeviceToHost, cs()));
    }
    HIP_TRY(hipStreamSynchronize(cs()));
    for (int64_t q = 0; q < n_q; ++q) cv[f.where[q]] = q_dec[q];
    for (size_t t = 0; t < np; ++t) {
        o.task_iterations[t * 6] = iters[t];
        o.task_status[t * 6] = st_words[t];
        for (int fold = 0; fold < 5; ++fold) {
            const int ft = f.fold_task[t * 5 + fold];
            o.task_iterations[t * 6 + 1 + fold] = ft < 0 ? 0 : iters[ft];
            o.task_status[t * 6 + 1 + fold] = ft < 0 ? 0 : st_words[ft];
        }
    }
    if (o.cv_dec) std::copy(cv.begin(), cv.end(), o.cv_dec);
    // the sigmoid of every pair: its held-out values in pair-row order with the signs of its full task
    DevBlock d_cv;
    BlockPart cv_part[] = {{cv.data(), rows_full * 8, 8}};
    if ((rc = block_upload(d_cv, cv_part, 1, "the held-out decision values"))) return rc;
    return platt_run((const double *)cv_part[0].dev, m.sign, (const long long *)parts[2].dev, (int)np, l_max, o.prob_a, o.prob_b,
                     o.sig_iterations, o.sig_stop);
}

// SVC(probability=True).fit for every job: the full fits, Platt's folds and the sigmoid fits; see paa_hip.h
// (use_cache false: paa_svc_fit_proba_f64; true: paa_svc_fit_proba_cached_f64 with its budget and flags: a job is a group)
static int svc_fit_proba_run(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs, const int64_t *train_off,
                             const int32_t *train_idx, const double *mean, const double *std, const double *C, const double *gamma,
                             int kernel_type, double eps, int max_iter, int iters_per_launch, const int64_t *seed, int n_pairs,
                             int64_t n_rows, double *alpha_y, double *rho, double *prob_a, double *prob_b, int32_t *n_sv,
                             int32_t *task_iterations, int32_t *task_status, int32_t *sig_iterations, int32_t *sig_stop, double *cv_dec,
                             int32_t *n_launches, bool use_cache, int64_t cache_bytes, int32_t *job_cached) {
    // check
    if (!X || !labels || !train_off || !train_idx || !mean || !std || !C || !gamma || !seed || !alpha_y || !rho || !prob_a || !prob_b ||
        !n_sv || !task_iterations || !task_status || !sig_iterations || !sig_stop || (use_cache && !job_cached))
        return fail(PAA_ERR_ARG, "null argument");
    int rc;
    if ((rc = sweep_samples_check(n_samples))) return rc;
    if ((rc = smo_params_check(n_dims, kernel_type, eps, max_iter, iters_per_launch))) return rc;
    if (n_jobs < 1) return fail(PAA_ERR_ARG, "no jobs");
    if ((rc = sweep_offsets_check(train_off, n_jobs, "train"))) return rc;
    const int64_t n_t = train_off[n_jobs];
    if ((rc = sweep_index_check(train_idx, n_t, n_samples, "train"))) return rc;
    for (int64_t i = 0; i < n_t; ++i)
        if (labels[train_idx[i]] < 0) return fail(PAA_ERR_ARG, "training sample %d has the label %d: class indices are >= 0", train_idx[i], labels[train_idx[i]]);
    for (int j = 0; j < n_jobs; ++j)
        if (seed[j] < 0 || seed[j] > 0x7fffffffLL) return fail(PAA_ERR_ARG, "job %d: seed %lld: libsvm's random_seed is in 0 .. 2^31 - 1", j, (long long)seed[j]);
    // the tasks: the full fit of every pair (the folds follow in svc_fit_proba_resident)
    PairTasks p;
    if ((rc = svc_pair_tasks(p, labels, n_jobs, train_off, train_idx, C, gamma, kernel_type))) return rc;
    if (n_pairs != (int)p.tasks.size() || n_rows != (int64_t)p.idx.size())
        return fail(PAA_ERR_ARG, "n_pairs = %d, n_rows = %lld: the jobs make %d pairs of %lld rows", n_pairs, (long long)n_rows, (int)p.tasks.size(), (long long)p.idx.size());
    if (use_cache && (rc = svr_cache_args_check(cache_bytes))) return rc;
    if ((rc = ensure_init())) return rc;
    // X goes up once, through the lane's scratch, with every job's mean and scale behind it
    const size_t sb = (size_t)n_jobs * n_dims * 8;
    DevBlock stats;
    BlockPart parts[] = {{mean, sb, 8}, {std, sb, 8}};
    if ((rc = block_upload(stats, parts, 2, "the probabilistic SVM jobs"))) return rc;
    Staged st;
    if ((rc = stage(st, X, n_dims, n_samples, nullptr, nullptr, 0, {}))) return rc;
    const ProbaFitOut o{alpha_y, rho, prob_a, prob_b, n_sv, task_iterations, task_status, sig_iterations, sig_stop, cv_dec, n_launches,
                        use_cache ? job_cached : nullptr, cache_bytes};
    return svc_fit_proba_resident(st.feats, (const double *)parts[0].dev, (const double *)parts[1].dev, n_dims, p, seed, kernel_type, eps,
                                  max_iter, iters_per_launch, o);
}
extern "C" int paa_svc_fit_proba_f64(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs,
                                     const int64_t *train_off, const int32_t *train_idx, const double *mean, const double *std,
                                     const double *C, const double *gamma, int kernel_type, double eps, int max_iter,
                                     int iters_per_launch, const int64_t *seed, int n_pairs, int64_t n_rows, double *alpha_y,
                                     double *rho, double *prob_a, double *prob_b, int32_t *n_sv, int32_t *task_iterations,
                                     int32_t *task_status, int32_t *sig_iterations, int32_t *sig_stop, double *cv_dec,
                                     int32_t *n_launches) {
    return svc_fit_proba_run(X, n_samples, n_dims, labels, n_jobs, train_off, train_idx, mean, std, C, gamma, kernel_type, eps, max_iter,
                             iters_per_launch, seed, n_pairs, n_rows, alpha_y, rho, prob_a, prob_b, n_sv, task_iterations, task_status,
                             sig_iterations, sig_stop, cv_dec, n_launches, false, 0, nullptr);
}
extern "C" int paa_svc_fit_proba_cached_f64(const double *X, int64_t n_samples, int n_dims, const int32_t *labels, int n_jobs,
                                            const int64_t *train_off, const int32_t *train_idx, const double *mean, const double *std,
                                            const double *C, const double *gamma, int kernel_type, double eps, int max_iter,
                                            int iters_per_launch, const int64_t *seed, int n_pairs, int64_t n_rows, double *alpha_y,
                                            double *rho, double *prob_a, double *prob_b, int32_t *n_sv, int32_t *task_iterations,
                                            int32_t *task_status, int32_t *sig_iterations, int32_t *sig_stop, double *cv_dec,
                                            int32_t *n_launches, int64_t cache_bytes, int32_t *job_cached) {
    return svc_fit_proba_run(X, n_samples, n_dims, labels, n_jobs, train_off, train_idx, mean, std, C, gamma, kernel_type, eps, max_iter,
                             iters_per_launch, seed, n_pairs, n_rows, alpha_y, rho, prob_a, prob_b, n_sv, task_iterations, task_status,
                             sig_iterations, sig_stop, cv_dec, n_launches, true, cache_bytes, job_cached);
}
