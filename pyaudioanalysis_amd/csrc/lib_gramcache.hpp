// The resident kernel matrices of the SMO solvers on the host (DESIGN K22, K23): the packing rule, the scratch of a call and the Gram pass
// (svr_standardise_kernel, svr_gram_kernel of kernels_svrcache.hpp, family_svr.hip).  A matrix runs over the rows of an smo::SmoTask:
// for the SVR solver (lib_svrfit.hpp) a task of the batch, for the C-SVC solver (lib_smo.hpp) the row list of a group of tasks.
#pragma once

// The packing rule of the resident matrices: the matrix of a task of n rows takes 8 n^2 bytes (its standardised rows and the tile list
// ride along uncounted).  In task order: a task whose matrix exceeds `cache_bytes` is not cached; any other joins the open chunk when
// the chunk's matrices and its own fit the budget together, and otherwise closes it and opens the next.  chunk_of [n_tasks]: the
// task's chunk from 0, -1 when it is not cached.  Returns the number of chunks
static int svr_cache_pack(const std::vector<smo::SmoTask> &tasks, int64_t cache_bytes, std::vector<int> &chunk_of) {
    chunk_of.assign(tasks.size(), -1);
    int n_chunks = 0;
    int64_t used = 0;
    for (size_t t = 0; t < tasks.size(); ++t) {
        const int64_t bytes = (int64_t)tasks[t].n * tasks[t].n * 8;
        if (bytes > cache_bytes) continue;
        if (n_chunks == 0 || used + bytes > cache_bytes) { ++n_chunks; used = 0; }
        used += bytes;
        chunk_of[t] = n_chunks - 1;
    }
    return n_chunks;
}

// The resident matrices of a call, freed on return: K | Z of the largest chunk, k_off | z_off [tasks], the chunk's task list and its
// tile pairs
struct SvrCache {
    DevBlock block;
    svrfit::SvrCacheDev dev{};
    int *chunk = nullptr;
    svrfit::GramTile *tiles = nullptr;
    std::vector<int> chunk_of;
    int n_chunks = 0;
    std::vector<long long> off;           // k_off | z_off on the host
};
static long long svr_tile_pairs(int n) {
    const long long nt = (n + svrfit::kGramTile - 1) / svrfit::kGramTile;
    return nt * (nt + 1) / 2;
}
// packs the tasks and allocates for the largest chunk (nothing when no task is cached)
static int svr_cache_alloc(SvrCache &c, const std::vector<smo::SmoTask> &tasks, int n_dims, int64_t cache_bytes) {
    const size_t n_tasks = tasks.size();
    c.n_chunks = svr_cache_pack(tasks, cache_bytes, c.chunk_of);
    if (!c.n_chunks) return PAA_OK;
    const long long pitch = (n_dims + svrfit::kPitchLanes - 1) / svrfit::kPitchLanes * svrfit::kPitchLanes;
    std::vector<long long> k_sum(c.n_chunks, 0), z_sum(c.n_chunks, 0), tile_sum(c.n_chunks, 0), count(c.n_chunks, 0);
    c.off.assign(2 * n_tasks, 0);
    for (size_t t = 0; t < n_tasks; ++t) {
        const int ch = c.chunk_of[t];
        if (ch < 0) continue;
        const long long n = tasks[t].n;
        c.off[t] = k_sum[ch];
        c.off[n_tasks + t] = z_sum[ch];
        k_sum[ch] += n * n;
        z_sum[ch] += n * pitch;
        tile_sum[ch] += svr_tile_pairs(tasks[t].n);
        ++count[ch];
    }
    const size_t b_k = up256((size_t)*std::max_element(k_sum.begin(), k_sum.end()) * 8);
    const size_t b_z = up256((size_t)*std::max_element(z_sum.begin(), z_sum.end()) * 8);
    const size_t b_off = up256(2 * n_tasks * 8), b_chunk = up256((size_t)*std::max_element(count.begin(), count.end()) * 4);
    const size_t b_tiles = (size_t)*std::max_element(tile_sum.begin(), tile_sum.end()) * sizeof(svrfit::GramTile);
    HIP_TRY(hipMalloc(&c.block.p, b_k + b_z + b_off + b_chunk + b_tiles));
    char *p = (char *)c.block.p;
    c.dev.K = (double *)p;                  p += b_k;
    c.dev.Z = (double *)p;                  p += b_z;
    c.dev.k_off = (const long long *)p;
    c.dev.z_off = (const long long *)p + n_tasks;
    HIP_TRY(hipMemcpyAsync(p, c.off.data(), 2 * n_tasks * 8, hipMemcpyHostToDevice, cs()));
    p += b_off;
    c.chunk = (int *)p;                     p += b_chunk;
    c.tiles = (svrfit::GramTile *)p;
    return PAA_OK;
}
// forms Z and K of chunk `ch`; `members` returns its tasks
static int svr_cache_fill(const SvrCache &c, const svrfit::SvrDev &m, const std::vector<smo::SmoTask> &tasks, int ch, std::vector<int> &members) {
    members.clear();
    std::vector<svrfit::GramTile> tiles;
    int n_max = 0;
    for (size_t t = 0; t < tasks.size(); ++t) {
        if (c.chunk_of[t] != ch) continue;
        members.push_back((int)t);
        n_max = std::max(n_max, tasks[t].n);
        const int nt = (tasks[t].n + svrfit::kGramTile - 1) / svrfit::kGramTile;
        for (int a = 0; a < nt; ++a)
            for (int b = a; b < nt; ++b) tiles.push_back({(int)t, a, b});
    }
    HIP_TRY(hipMemcpy(c.chunk, members.data(), members.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c.tiles, tiles.data(), tiles.size() * sizeof(svrfit::GramTile), hipMemcpyHostToDevice));
    LAUNCH_TRY("SVR Gram", launch::svr_gram(m, c.dev, c.chunk, (int)members.size(), n_max, c.tiles, (long long)tiles.size(), cs()));
    return PAA_OK;
}
static int svr_cache_args_check(int64_t cache_bytes) {
    if (cache_bytes <= 0) return fail(PAA_ERR_ARG, "cache_bytes = %lld: a positive budget is needed", (long long)cache_bytes);
    return PAA_OK;
}
