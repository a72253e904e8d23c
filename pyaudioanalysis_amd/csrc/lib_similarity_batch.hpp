// Host entry points of the batched self-similarity matrix / thumbnail filter (audioSegmentation.music_thumbnailing over a
// collection of clips) over kernels_simbatch.hpp: the host builds per-clip records and the tile / block lists, every stage of
// all clips of a chunk is one launch, and the arg-max cell is grown on the device -- 48 bytes per clip come back, plus the
// filtered matrices when they are asked for.  Whole clips are taken in chunks that keep the device scratch of a chunk within
// 1 GiB; no result depends on the chunking.  One of the units paa_lib.hip is made of.
#pragma once

constexpr int64_t kSimbMaxVec = 46340LL * 4;      // paa_dev_self_similarity's size bound
static std::mutex g_simb_mu;                      // the scratch and the staging buffers below: one enqueue sequence at a time
static GlobalScratch g_simb_z, g_simb_aux, g_simb_cand;                               // device entry points
static GlobalScratch g_simb_in, g_simb_feat, g_simb_sim, g_simb_filt, g_simb_res;     // host-buffer entry points

// The records and lists of one call travel through a pinned host buffer, so that the copy is asynchronous and the entry point
// does not wait for the stream; the event tells when the buffer may be written again.
struct SimbStage {
    void *h = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
    GlobalScratch dev;
};
static SimbStage g_simb_stage_sim, g_simb_stage_thumb;
static int simb_stage_begin(SimbStage &s, size_t bytes) {
    if (s.pending) {
        HIP_TRY(hipEventSynchronize(s.ev));
        s.pending = false;
    }
    if (!s.ev) HIP_TRY(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    if (bytes > s.cap) {
        if (s.h) (void)hipHostFree(s.h);
        s.h = nullptr;
        s.cap = 0;
        const size_t want = bytes + bytes / 8 + 4096;
        HIP_TRY(hipHostMalloc(&s.h, want, hipHostMallocDefault));
        s.cap = want;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    return scratch_reserve(s.dev, bytes);
}
static int simb_stage_send(SimbStage &s, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(s.dev.p, s.h, bytes, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipEventRecord(s.ev, cs()));
    s.pending = true;
    return PAA_OK;
}
// paa_shutdown: the pinned buffers and events belong to the device that goes away (the device halves are GlobalScratch)
static void simb_release() {
    std::lock_guard<std::mutex> lk(g_simb_mu);
    for (SimbStage *s : {&g_simb_stage_sim, &g_simb_stage_thumb}) {
        if (s->ev) (void)hipEventDestroy(s->ev);
        if (s->h) (void)hipHostFree(s->h);
        s->ev = nullptr;
        s->h = nullptr;
        s->cap = 0;
        s->pending = false;
    }
}

// ------------------------------------------------------------------------------------------
// host-built layouts (no device): per-clip records, tile list, block lists
// ------------------------------------------------------------------------------------------
struct SimbSimLayout {
    std::vector<simb::SimClip> clips;
    std::vector<simb::SimTile> tiles;       // (clip, ti <= tj), clip-major, rows of the triangle in order
    long long z_doubles = 0, aux_doubles = 0, max_ldz = 0;
};
static void simb_sim_layout(int n_dims, int64_t n_clips, const int64_t *feat_off, const int64_t *n_vec, const int64_t *ld,
                            const int64_t *sim_off, SimbSimLayout &L) {
    const long long dims_pad = (n_dims + 3) / 4 * 4;
    L.clips.resize((size_t)n_clips);
    for (int64_t c = 0; c < n_clips; ++c) {
        const long long T = n_vec[c], ldz = (T + kSimTile - 1) / kSimTile * kSimTile, tiles = ldz / kSimTile;
        L.clips[c] = simb::SimClip{feat_off ? feat_off[c] : 0, ld ? ld[c] : T, T, ldz, L.z_doubles, L.aux_doubles, sim_off ? sim_off[c] : 0};
        L.z_doubles += dims_pad * ldz;
        L.aux_doubles += 2LL * n_dims + ldz;
        L.max_ldz = std::max(L.max_ldz, ldz);
        for (long long ti = 0; ti < tiles; ++ti)
            for (long long tj = ti; tj < tiles; ++tj) L.tiles.push_back(simb::SimTile{(int)c, (int)ti, (int)tj, 0});
    }
}

struct SimbThumbLayout {
    std::vector<simb::ThumbClip> clips;
    std::vector<simb::ThumbBlock> blocks;   // thumb_diag blocks that hold a cell
    std::vector<simb::ThumbBlock> rows;     // thumb_fill row blocks (bx unused)
    long long cand_words = 0, max_R = 0;
};
static void simb_thumb_layout(int64_t n_clips, const int64_t *sim_off, const int64_t *n_vec, int m_filter, double limit_1,
                              double limit_2, const int64_t *filt_off, SimbThumbLayout &L) {
    L.clips.resize((size_t)n_clips);
    for (int64_t c = 0; c < n_clips; ++c) {
        const long long T = n_vec[c], R = T - m_filter + 1;
        const long long gx = (R + 255) / 256, gy = (R + kDiagRun - 1) / kDiagRun, my = (R + kMaskRows - 1) / kMaskRows;
        L.clips[c] = simb::ThumbClip{sim_off ? sim_off[c] : 0, filt_off ? filt_off[c] : 0, L.cand_words, T, R,
                                     (long long)(limit_1 * (double)R), (long long)(limit_2 * (double)R), (int)gx, (int)gy};   // int(), :1157-1160
        L.cand_words += 3 * gx * gy + 2;
        L.max_R = std::max(L.max_R, R);
        for (long long by = 0; by < gy; ++by)
            for (long long bx = 0; bx < gx && simb::diag_block_live(bx, by, R); ++bx)
                L.blocks.push_back(simb::ThumbBlock{(int)c, (int)bx, (int)by, 0});
        for (long long by = 0; by < my; ++by) L.rows.push_back(simb::ThumbBlock{(int)c, 0, (int)by, 0});
    }
}

// ------------------------------------------------------------------------------------------
// argument checks (before the device is touched)
// ------------------------------------------------------------------------------------------
static int simb_check_vectors(int n_dims, int64_t n_clips, const int64_t *n_vec) {
    if (n_clips < 1 || n_clips > 0x3fffffffLL) return fail(PAA_ERR_ARG, "%lld clips", (long long)n_clips);
    if (n_dims < 1 || n_dims > 65535) return fail(PAA_ERR_ARG, "feature matrices of %d rows", n_dims);
    for (int64_t c = 0; c < n_clips; ++c) {
        if (n_vec[c] < 1) return fail(PAA_ERR_ARG, "clip %lld: empty feature matrix (%lld vectors)", (long long)c, (long long)n_vec[c]);
        if (n_vec[c] > kSimbMaxVec)
            return fail(PAA_ERR_UNSUPPORTED, "clip %lld: %lld vectors: similarity matrix too large", (long long)c, (long long)n_vec[c]);
    }
    if (n_clips * (int64_t)n_dims > 0x7fffffffLL) return fail(PAA_ERR_UNSUPPORTED, "%lld clips of %d rows: too many for one launch", (long long)n_clips, n_dims);
    return PAA_OK;
}
static int simb_check_filter(int64_t n_clips, const int64_t *n_vec, int m_filter, double limit_1, double limit_2) {
    if (n_clips < 1 || n_clips > 0x3fffffffLL) return fail(PAA_ERR_ARG, "%lld clips", (long long)n_clips);
    if (m_filter < 1) return fail(PAA_ERR_ARG, "thumbnail filter length %d", m_filter);
    if (!(limit_1 >= 0.0) || !(limit_2 >= 0.0)) return fail(PAA_ERR_ARG, "limit_1 / limit_2 must be >= 0");
    for (int64_t c = 0; c < n_clips; ++c) {
        if (n_vec[c] < m_filter)
            return fail(PAA_ERR_ARG, "clip %lld: fewer feature vectors (%lld) than the thumbnail filter length (%d)", (long long)c,
                        (long long)n_vec[c], m_filter);
        if (n_vec[c] > kSimbMaxVec)
            return fail(PAA_ERR_UNSUPPORTED, "clip %lld: %lld vectors: similarity matrix too large", (long long)c, (long long)n_vec[c]);
    }
    return PAA_OK;
}

// ------------------------------------------------------------------------------------------
// device buffers in and out
// ------------------------------------------------------------------------------------------
extern "C" int paa_dev_self_similarity_batch(const double *d_feats, int n_dims, int64_t n_clips, const int64_t *feat_off,
                                             const int64_t *n_vec, const int64_t *ld, double *d_sim, const int64_t *sim_off) {
    if (!d_feats || !d_sim || !feat_off || !n_vec || !ld || !sim_off) return fail(PAA_ERR_ARG, "null buffer");
    int rc = simb_check_vectors(n_dims, n_clips, n_vec);
    if (rc) return rc;
    for (int64_t c = 0; c < n_clips; ++c)
        if (feat_off[c] < 0 || sim_off[c] < 0 || ld[c] < n_vec[c])
            return fail(PAA_ERR_ARG, "clip %lld: bad feature matrix placement (offsets %lld / %lld, %lld vectors, ld %lld)", (long long)c,
                        (long long)feat_off[c], (long long)sim_off[c], (long long)n_vec[c], (long long)ld[c]);
    if ((rc = ensure_init())) return rc;
    std::lock_guard<std::mutex> lk(g_simb_mu);
    SimbSimLayout L;
    simb_sim_layout(n_dims, n_clips, feat_off, n_vec, ld, sim_off, L);
    const int dims_pad = (n_dims + 3) / 4 * 4;
    {
        std::lock_guard<std::mutex> lk2(g_mu);
        if ((rc = scratch_reserve(g_simb_z, (size_t)L.z_doubles * 8))) return rc;
        if ((rc = scratch_reserve(g_simb_aux, (size_t)L.aux_doubles * 8))) return rc;
    }
    const size_t b_clips = up256(L.clips.size() * sizeof(simb::SimClip)), b_tiles = L.tiles.size() * sizeof(simb::SimTile);
    SimbStage &st = g_simb_stage_sim;
    if ((rc = simb_stage_begin(st, b_clips + b_tiles))) return rc;
    memcpy(st.h, L.clips.data(), L.clips.size() * sizeof(simb::SimClip));
    memcpy((char *)st.h + b_clips, L.tiles.data(), b_tiles);
    if ((rc = simb_stage_send(st, b_clips + b_tiles))) return rc;
    const simb::SimClip *d_clips = (const simb::SimClip *)st.dev.p;
    const simb::SimTile *d_tiles = (const simb::SimTile *)((const char *)st.dev.p + b_clips);
    double *d_aux = (double *)g_simb_aux.p, *d_z = (double *)g_simb_z.p;
    hipLaunchKernelGGL(simb::sim_row_stats_batch_kernel, dim3((unsigned)(n_clips * n_dims)), dim3(256), 0, cs(), d_feats, d_clips,
                       n_dims, d_aux);
    hipLaunchKernelGGL(simb::sim_normalize_batch_kernel, dim3((unsigned)n_clips, (unsigned)((L.max_ldz + 255) / 256)), dim3(256), 0,
                       cs(), d_feats, d_clips, n_dims, dims_pad, d_aux, d_z);
    const size_t lds = (size_t)2 * kSimChunk * kSimPitch * 8 + 256 * 8;
    static LdsAttrCache attr;
    if (!attr.covers(lds)) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&simb::sim_gram_batch_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr.set(lds);
    }
    const long long n_tiles = (long long)L.tiles.size();
    const dim3 gram_grid((unsigned)std::min<long long>(n_tiles, 2LL * g_num_cu));       // two workgroups per CU, as the single call
    hipLaunchKernelGGL(simb::sim_gram_batch_kernel, gram_grid, dim3(512), lds, cs(), (const double *)d_z, dims_pad, n_dims, d_clips,
                       d_tiles, n_tiles, (const double *)d_aux, d_sim);
    HIP_TRY(hipGetLastError());
    return PAA_OK;
}

extern "C" int paa_dev_thumbnail_filter_batch(const double *d_sim, const int64_t *sim_off, const int64_t *n_vec, int64_t n_clips,
                                              int m_filter, double band, double limit_1, double limit_2, double *d_filt,
                                              const int64_t *filt_off, int64_t *d_pos, int64_t *d_bounds) {
    if (!d_sim || !sim_off || !n_vec || !d_filt || !filt_off || !d_pos || !d_bounds) return fail(PAA_ERR_ARG, "null buffer");
    int rc = simb_check_filter(n_clips, n_vec, m_filter, limit_1, limit_2);
    if (rc) return rc;
    for (int64_t c = 0; c < n_clips; ++c)
        if (sim_off[c] < 0 || filt_off[c] < 0)
            return fail(PAA_ERR_ARG, "clip %lld: negative offset (%lld / %lld)", (long long)c, (long long)sim_off[c], (long long)filt_off[c]);
    if ((rc = ensure_init())) return rc;
    std::lock_guard<std::mutex> lk(g_simb_mu);
    SimbThumbLayout L;
    simb_thumb_layout(n_clips, sim_off, n_vec, m_filter, limit_1, limit_2, filt_off, L);
    if (L.blocks.size() > 0x7fffffffULL || L.rows.size() > 0x7fffffffULL)
        return fail(PAA_ERR_UNSUPPORTED, "%zu diagonal blocks: too many for one launch", L.blocks.size());
    {
        std::lock_guard<std::mutex> lk2(g_mu);
        if ((rc = scratch_reserve(g_simb_cand, (size_t)L.cand_words * 8))) return rc;
    }
    const size_t b_clips = up256(L.clips.size() * sizeof(simb::ThumbClip)), b_blocks = up256(L.blocks.size() * sizeof(simb::ThumbBlock)),
                 b_rows = L.rows.size() * sizeof(simb::ThumbBlock);
    SimbStage &st = g_simb_stage_thumb;
    if ((rc = simb_stage_begin(st, b_clips + b_blocks + b_rows))) return rc;
    memcpy(st.h, L.clips.data(), L.clips.size() * sizeof(simb::ThumbClip));
    memcpy((char *)st.h + b_clips, L.blocks.data(), L.blocks.size() * sizeof(simb::ThumbBlock));
    memcpy((char *)st.h + b_clips + b_blocks, L.rows.data(), b_rows);
    if ((rc = simb_stage_send(st, b_clips + b_blocks + b_rows))) return rc;
    const simb::ThumbClip *d_clips = (const simb::ThumbClip *)st.dev.p;
    const simb::ThumbBlock *d_blocks = (const simb::ThumbBlock *)((const char *)st.dev.p + b_clips);
    const simb::ThumbBlock *d_rows = (const simb::ThumbBlock *)((const char *)st.dev.p + b_clips + b_blocks);
    double *d_cand = (double *)g_simb_cand.p;
    hipLaunchKernelGGL(simb::thumb_diag_batch_kernel, dim3((unsigned)L.blocks.size()), dim3(256), 0, cs(), d_sim, d_clips, d_blocks,
                       m_filter, band, d_filt, d_cand);
    hipLaunchKernelGGL(simb::thumb_min_batch_kernel, dim3((unsigned)n_clips), dim3(1024), 0, cs(), d_clips, d_cand);
    hipLaunchKernelGGL(simb::thumb_fill_batch_kernel, dim3((unsigned)L.rows.size(), (unsigned)((L.max_R + 1023) / 1024)), dim3(256), 0,
                       cs(), d_clips, d_rows, band, d_filt, (const double *)d_cand);
    hipLaunchKernelGGL(simb::thumb_argmax_batch_kernel, dim3((unsigned)n_clips), dim3(1024), 0, cs(), d_clips, band, d_cand,
                       (long long *)d_pos);
    hipLaunchKernelGGL(simb::thumb_grow_batch_kernel, dim3((unsigned)((n_clips + 63) / 64)), dim3(64), 0, cs(), d_clips,
                       (long long)n_clips, m_filter, (const double *)d_filt, (const long long *)d_pos, (long long *)d_bounds);
    HIP_TRY(hipGetLastError());
    return PAA_OK;
}

// ------------------------------------------------------------------------------------------
// host buffers in and out, in chunks of whole clips
// ------------------------------------------------------------------------------------------
// the device scratch a clip of T vectors can need: its input, Z and norms, both matrices, candidates, lists
static size_t simb_clip_bytes(long long T, int n_dims, int m_filter, size_t input_bytes) {
    const long long ldz = (T + kSimTile - 1) / kSimTile * kSimTile, tiles = ldz / kSimTile, dims_pad = (n_dims + 3) / 4 * 4;
    size_t b = input_bytes + (size_t)(dims_pad * ldz + 2LL * n_dims + ldz + T * T) * 8 + (size_t)(tiles * (tiles + 1) / 2) * 16 + 4096;
    if (m_filter > 0 && T >= m_filter) {
        const long long R = T - m_filter + 1, gx = (R + 255) / 256, gy = (R + kDiagRun - 1) / kDiagRun;
        b += (size_t)(R * R + 3 * gx * gy + 2 + 6) * 8 + (size_t)(gx * gy + (R + kMaskRows - 1) / kMaskRows) * 16;
    }
    return b;
}

struct SimbHostOut {
    double *sim = nullptr;        // T_c x T_c matrices back to back, or null
    double *filt = nullptr;       // R_c x R_c matrices back to back, or null
    int64_t *pos = nullptr;       // [n][2]
    int64_t *bounds = nullptr;    // [n][4]
};
// prefix sums of T^2 and R^2 over the clips (doubles)
static void simb_prefixes(int64_t n_clips, const int64_t *n_vec, int m_filter, std::vector<int64_t> &sim_pref, std::vector<int64_t> &filt_pref) {
    sim_pref.assign((size_t)n_clips + 1, 0);
    filt_pref.assign((size_t)n_clips + 1, 0);
    for (int64_t c = 0; c < n_clips; ++c) {
        const int64_t R = m_filter > 0 ? n_vec[c] - m_filter + 1 : 0;
        sim_pref[c + 1] = sim_pref[c] + n_vec[c] * n_vec[c];
        filt_pref[c + 1] = filt_pref[c] + R * R;
    }
}
// The stages of clips [c0, c1) and their copy-back.  d_feats: the chunk's feature matrices (clip c at feat_off[c - c0] with
// pitch ld[c - c0]), or null when g_simb_sim already holds the chunk's similarity matrices back to back.  m_filter = 0 stops
// after the similarity stage.  Drains the stream before it returns.
static int simb_chunk_stages(const double *d_feats, const int64_t *feat_off, const int64_t *ld, int n_dims, int c0, int c1,
                             const int64_t *n_vec, const std::vector<int64_t> &sim_pref, const std::vector<int64_t> &filt_pref,
                             int m_filter, double band, double limit_1, double limit_2, const SimbHostOut &o) {
    const int n = c1 - c0;
    int rc;
    std::vector<int64_t> sim_off((size_t)n), filt_off((size_t)n);
    for (int c = 0; c < n; ++c) {
        sim_off[c] = sim_pref[c0 + c] - sim_pref[c0];
        filt_off[c] = filt_pref[c0 + c] - filt_pref[c0];
    }
    const size_t sim_doubles = (size_t)(sim_pref[c1] - sim_pref[c0]), filt_doubles = (size_t)(filt_pref[c1] - filt_pref[c0]);
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if ((rc = scratch_reserve(g_simb_sim, sim_doubles * 8))) return rc;
        if (m_filter > 0) {
            if ((rc = scratch_reserve(g_simb_filt, filt_doubles * 8))) return rc;
            if ((rc = scratch_reserve(g_simb_res, (size_t)n * 6 * 8))) return rc;
        }
    }
    if (d_feats && (rc = paa_dev_self_similarity_batch(d_feats, n_dims, n, feat_off, n_vec + c0, ld, (double *)g_simb_sim.p, sim_off.data())))
        return rc;
    if (o.sim) HIP_TRY(hipMemcpyAsync(o.sim + sim_pref[c0], g_simb_sim.p, sim_doubles * 8, hipMemcpyDeviceToHost, cs()));
    if (m_filter > 0) {
        int64_t *d_pos = (int64_t *)g_simb_res.p, *d_bounds = d_pos + 2 * (size_t)n;
        if ((rc = paa_dev_thumbnail_filter_batch((const double *)g_simb_sim.p, sim_off.data(), n_vec + c0, n, m_filter, band, limit_1,
                                                 limit_2, (double *)g_simb_filt.p, filt_off.data(), d_pos, d_bounds)))
            return rc;
        if (o.filt) HIP_TRY(hipMemcpyAsync(o.filt + filt_pref[c0], g_simb_filt.p, filt_doubles * 8, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(o.pos + 2 * (size_t)c0, d_pos, (size_t)n * 16, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(o.bounds + 4 * (size_t)c0, d_bounds, (size_t)n * 32, hipMemcpyDeviceToHost, cs()));
    }
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}

// packed feature matrices (clip after clip, each [n_dims][T_c] row-major) through the stages
static int simb_run_features(const double *feats, int n_dims, int64_t n_clips, const int64_t *n_vec, int m_filter, double band,
                             double limit_1, double limit_2, int64_t chunk_bytes, const SimbHostOut &o) {
    int rc;
    std::vector<int64_t> sim_pref, filt_pref, in_pref((size_t)n_clips + 1, 0);
    simb_prefixes(n_clips, n_vec, m_filter, sim_pref, filt_pref);
    std::vector<size_t> bytes((size_t)n_clips);
    for (int64_t c = 0; c < n_clips; ++c) {
        in_pref[c + 1] = in_pref[c] + (int64_t)n_dims * n_vec[c];
        bytes[c] = simb_clip_bytes(n_vec[c], n_dims, m_filter, (size_t)n_dims * n_vec[c] * 8);
    }
    if ((rc = ensure_init())) return rc;
    std::lock_guard<std::mutex> api_lock(g_api_mu);
    for (const auto &ch : onset_chunks(bytes, chunk_bytes)) {
        const int c0 = ch.first, c1 = ch.second, n = c1 - c0;
        const size_t in_doubles = (size_t)(in_pref[c1] - in_pref[c0]);
        {
            std::lock_guard<std::mutex> lk(g_mu);
            if ((rc = scratch_reserve(g_simb_in, in_doubles * 8))) return rc;
        }
        std::vector<int64_t> feat_off((size_t)n);
        for (int c = 0; c < n; ++c) feat_off[c] = in_pref[c0 + c] - in_pref[c0];
        HIP_TRY(hipMemcpyAsync(g_simb_in.p, feats + in_pref[c0], in_doubles * 8, hipMemcpyHostToDevice, cs()));
        if ((rc = simb_chunk_stages((const double *)g_simb_in.p, feat_off.data(), n_vec + c0, n_dims, c0, c1, n_vec, sim_pref, filt_pref,
                                    m_filter, band, limit_1, limit_2, o)))
            return rc;
    }
    return PAA_OK;
}

extern "C" int paa_self_similarity_batch_f64(const double *feats, int n_dims, int64_t n_clips, const int64_t *n_vec, int64_t chunk_bytes,
                                             double *sim) {
    if (!feats || !n_vec || !sim) return fail(PAA_ERR_ARG, "null buffer");
    const int rc = simb_check_vectors(n_dims, n_clips, n_vec);
    if (rc) return rc;
    SimbHostOut o;
    o.sim = sim;
    return simb_run_features(feats, n_dims, n_clips, n_vec, 0, 0.0, 0.0, 0.0, chunk_bytes, o);
}

extern "C" int paa_thumbnail_batch_f64(const double *feats, int n_dims, int64_t n_clips, const int64_t *n_vec, int m_filter, double band,
                                       double limit_1, double limit_2, int64_t chunk_bytes, int64_t *pos, int64_t *bounds, double *filt) {
    if (!feats || !n_vec || !pos || !bounds) return fail(PAA_ERR_ARG, "null buffer");
    int rc = simb_check_vectors(n_dims, n_clips, n_vec);
    if (rc) return rc;
    if ((rc = simb_check_filter(n_clips, n_vec, m_filter, limit_1, limit_2))) return rc;
    SimbHostOut o;
    o.filt = filt;
    o.pos = pos;
    o.bounds = bounds;
    return simb_run_features(feats, n_dims, n_clips, n_vec, m_filter, band, limit_1, limit_2, chunk_bytes, o);
}

// packed similarity matrices (T_c x T_c, back to back) through the filter stages alone
extern "C" int paa_thumbnail_filter_batch_f64(const double *sims, int64_t n_clips, const int64_t *n_vec, int m_filter, double band,
                                              double limit_1, double limit_2, int64_t chunk_bytes, int64_t *pos, int64_t *bounds,
                                              double *filt) {
    if (!sims || !n_vec || !pos || !bounds) return fail(PAA_ERR_ARG, "null buffer");
    int rc = simb_check_filter(n_clips, n_vec, m_filter, limit_1, limit_2);
    if (rc) return rc;
    std::vector<int64_t> sim_pref, filt_pref;
    simb_prefixes(n_clips, n_vec, m_filter, sim_pref, filt_pref);
    std::vector<size_t> bytes((size_t)n_clips);
    for (int64_t c = 0; c < n_clips; ++c) bytes[c] = simb_clip_bytes(n_vec[c], 1, m_filter, 0);
    if ((rc = ensure_init())) return rc;
    std::lock_guard<std::mutex> api_lock(g_api_mu);
    SimbHostOut o;
    o.filt = filt;
    o.pos = pos;
    o.bounds = bounds;
    for (const auto &ch : onset_chunks(bytes, chunk_bytes)) {
        const int c0 = ch.first, c1 = ch.second;
        const size_t sim_doubles = (size_t)(sim_pref[c1] - sim_pref[c0]);
        {
            std::lock_guard<std::mutex> lk(g_mu);
            if ((rc = scratch_reserve(g_simb_sim, sim_doubles * 8))) return rc;
        }
        HIP_TRY(hipMemcpyAsync(g_simb_sim.p, sims + sim_pref[c0], sim_doubles * 8, hipMemcpyHostToDevice, cs()));
        if ((rc = simb_chunk_stages(nullptr, nullptr, nullptr, 1, c0, c1, n_vec, sim_pref, filt_pref, m_filter, band, limit_1, limit_2, o)))
            return rc;
    }
    return PAA_OK;
}

// ------------------------------------------------------------------------------------------
// end to end: samples -> short-term features (one plan per chunk, 68 rows) -> stages 1 to 5 on the plan's slabs
// ------------------------------------------------------------------------------------------
// packed: the clips back to back, or null with clip_ptrs [n_clips]: every clip where the caller has it (no packing copy on the host)
static int run_thumbnail_batch(const void *packed, const void *const *clip_ptrs, const int64_t *offsets, int64_t n_clips, int sample_kind,
                               double fs, int window, int step, int m_filter, double band, double limit_1, double limit_2,
                               int64_t chunk_bytes, int64_t *pos, int64_t *bounds, double *filt) {
    if ((!packed && !clip_ptrs) || !offsets || !pos || !bounds) return fail(PAA_ERR_ARG, "null buffer");
    if (n_clips < 1 || n_clips > 0x3fffffffLL) return fail(PAA_ERR_ARG, "%lld clips", (long long)n_clips);
    if (window < 2 || step < 1) return fail(PAA_ERR_ARG, "window=%d step=%d: need window >= 2, step >= 1", window, step);
    const int n_dims = 2 * kBase;
    const size_t esz = sample_kind == 0 ? 2 : 8;
    std::vector<int64_t> n_vec((size_t)n_clips);
    for (int64_t c = 0; c < n_clips; ++c) {
        const int64_t len = offsets[c + 1] - offsets[c];
        if (len < 0) return fail(PAA_ERR_ARG, "clip %lld: offsets do not ascend (%lld after %lld)", (long long)c, (long long)offsets[c + 1], (long long)offsets[c]);
        if (clip_ptrs && !clip_ptrs[c]) return fail(PAA_ERR_ARG, "clip %lld: null buffer", (long long)c);
        n_vec[c] = paa_num_frames(len, window, step);
        if (n_vec[c] < 1)
            return fail(PAA_ERR_ARG, "clip %lld: need at least one array to concatenate (%lld samples, a window of %d)", (long long)c, (long long)len, window);
    }
    int rc = simb_check_filter(n_clips, n_vec.data(), m_filter, limit_1, limit_2);
    if (rc) return rc;
    std::vector<int64_t> sim_pref, filt_pref;
    simb_prefixes(n_clips, n_vec.data(), m_filter, sim_pref, filt_pref);
    std::vector<size_t> bytes((size_t)n_clips);
    for (int64_t c = 0; c < n_clips; ++c)
        bytes[c] = simb_clip_bytes(n_vec[c], n_dims, m_filter, (size_t)(offsets[c + 1] - offsets[c]) * esz + (size_t)n_dims * n_vec[c] * 8);
    if ((rc = ensure_init())) return rc;
    std::lock_guard<std::mutex> api_lock(g_api_mu);
    SimbHostOut o;
    o.filt = filt;
    o.pos = pos;
    o.bounds = bounds;
    for (const auto &ch : onset_chunks(bytes, chunk_bytes)) {
        const int c0 = ch.first, c1 = ch.second, n = c1 - c0;
        std::vector<int64_t> off((size_t)n + 1), feat_off((size_t)n);
        for (int c = 0; c <= n; ++c) off[c] = offsets[c0 + c] - offsets[c0];
        paa_plan *plan = nullptr;
        {
            std::lock_guard<std::mutex> lk(g_mu);
            rc = plan_build(off.data(), n, sample_kind, fs, window, step, 1, 0, &plan);
        }
        if (rc) return rc;
        std::unique_ptr<paa_plan, void (*)(paa_plan *)> guard(plan, plan_free_synced);
        {
            std::lock_guard<std::mutex> lk(g_mu);
            if ((rc = scratch_reserve(g_simb_in, (size_t)off[n] * esz + 64))) return rc;
            if ((rc = scratch_reserve(g_simb_feat, (size_t)plan->out_doubles * 8))) return rc;
        }
        if (packed) {
            HIP_TRY(hipMemcpyAsync(g_simb_in.p, (const char *)packed + (size_t)offsets[c0] * esz, (size_t)off[n] * esz, hipMemcpyHostToDevice, cs()));
        } else {
            for (int c = 0; c < n; ++c)
                HIP_TRY(hipMemcpyAsync((char *)g_simb_in.p + (size_t)off[c] * esz, clip_ptrs[c0 + c], (size_t)(off[c + 1] - off[c]) * esz,
                                       hipMemcpyHostToDevice, cs()));
        }
        if ((rc = paa_plan_execute(plan, g_simb_in.p, (double *)g_simb_feat.p))) return rc;
        for (int c = 0; c < n; ++c) {
            if (plan->clips[c].T != n_vec[c0 + c])
                return fail(PAA_ERR_ARG, "clip %d: %d frames in the plan, %lld expected", c0 + c, plan->clips[c].T, (long long)n_vec[c0 + c]);
            feat_off[c] = plan->clips[c].out_off;
        }
        if ((rc = simb_chunk_stages((const double *)g_simb_feat.p, feat_off.data(), n_vec.data() + c0, n_dims, c0, c1, n_vec.data(), sim_pref,
                                    filt_pref, m_filter, band, limit_1, limit_2, o)))
            return rc;
    }
    return PAA_OK;
}

// music_thumbnailing for a batch of clips: see paa_hip.h
extern "C" int paa_music_thumbnail_batch_i16(const int16_t *packed, const int64_t *offsets, int64_t n_clips, double fs, int window, int step,
                                             int m_filter, double band, double limit_1, double limit_2, int64_t chunk_bytes, int64_t *pos,
                                             int64_t *bounds, double *filt) {
    return run_thumbnail_batch(packed, nullptr, offsets, n_clips, 0, fs, window, step, m_filter, band, limit_1, limit_2, chunk_bytes, pos, bounds, filt);
}
extern "C" int paa_music_thumbnail_batch_f64(const double *packed, const int64_t *offsets, int64_t n_clips, double fs, int window, int step,
                                             int m_filter, double band, double limit_1, double limit_2, int64_t chunk_bytes, int64_t *pos,
                                             int64_t *bounds, double *filt) {
    return run_thumbnail_batch(packed, nullptr, offsets, n_clips, 1, fs, window, step, m_filter, band, limit_1, limit_2, chunk_bytes, pos, bounds, filt);
}
// the same with one pointer per clip instead of a packed array (offsets still give the lengths): a collection that sits in memory
// clip by clip is not copied together on the host first
extern "C" int paa_music_thumbnail_batch_ptrs_i16(const int16_t *const *clips, const int64_t *offsets, int64_t n_clips, double fs, int window,
                                                  int step, int m_filter, double band, double limit_1, double limit_2, int64_t chunk_bytes,
                                                  int64_t *pos, int64_t *bounds, double *filt) {
    return run_thumbnail_batch(nullptr, (const void *const *)clips, offsets, n_clips, 0, fs, window, step, m_filter, band, limit_1, limit_2,
                               chunk_bytes, pos, bounds, filt);
}
extern "C" int paa_music_thumbnail_batch_ptrs_f64(const double *const *clips, const int64_t *offsets, int64_t n_clips, double fs, int window,
                                                  int step, int m_filter, double band, double limit_1, double limit_2, int64_t chunk_bytes,
                                                  int64_t *pos, int64_t *bounds, double *filt) {
    return run_thumbnail_batch(nullptr, (const void *const *)clips, offsets, n_clips, 1, fs, window, step, m_filter, band, limit_1, limit_2,
                               chunk_bytes, pos, bounds, filt);
}

// ------------------------------------------------------------------------------------------
// introspection for the tests (host only): the layout a batch of these clips gets
// ------------------------------------------------------------------------------------------
// counts [3] = tiles, diagonal blocks, fill row blocks; tiles / blocks / rows [cap][3] = (clip, ti, tj) / (clip, bx, by) /
// (clip, 0, by); clip_off [n][3] = z_off, aux_off, cand_off.  A list longer than its capacity is an argument error.
extern "C" int paa_debug_thumbnail_batch_layout(const int64_t *n_vec, int64_t n_clips, int n_dims, int m_filter, int64_t *counts,
                                                int32_t *tiles, int64_t tiles_cap, int32_t *blocks, int64_t blocks_cap, int32_t *rows,
                                                int64_t rows_cap, int64_t *clip_off) {
    if (!n_vec || !counts || !tiles || !blocks || !rows || !clip_off) return fail(PAA_ERR_ARG, "null buffer");
    int rc = simb_check_vectors(n_dims, n_clips, n_vec);
    if (rc) return rc;
    if ((rc = simb_check_filter(n_clips, n_vec, m_filter, 0.0, 1.0))) return rc;
    SimbSimLayout S;
    SimbThumbLayout T;
    simb_sim_layout(n_dims, n_clips, nullptr, n_vec, nullptr, nullptr, S);
    simb_thumb_layout(n_clips, nullptr, n_vec, m_filter, 0.0, 1.0, nullptr, T);
    counts[0] = (int64_t)S.tiles.size();
    counts[1] = (int64_t)T.blocks.size();
    counts[2] = (int64_t)T.rows.size();
    if (counts[0] > tiles_cap || counts[1] > blocks_cap || counts[2] > rows_cap)
        return fail(PAA_ERR_ARG, "lists of %lld / %lld / %lld entries do not fit", (long long)counts[0], (long long)counts[1], (long long)counts[2]);
    for (size_t i = 0; i < S.tiles.size(); ++i) { tiles[3 * i] = S.tiles[i].clip; tiles[3 * i + 1] = S.tiles[i].ti; tiles[3 * i + 2] = S.tiles[i].tj; }
    for (size_t i = 0; i < T.blocks.size(); ++i) { blocks[3 * i] = T.blocks[i].clip; blocks[3 * i + 1] = T.blocks[i].bx; blocks[3 * i + 2] = T.blocks[i].by; }
    for (size_t i = 0; i < T.rows.size(); ++i) { rows[3 * i] = T.rows[i].clip; rows[3 * i + 1] = T.rows[i].bx; rows[3 * i + 2] = T.rows[i].by; }
    for (int64_t c = 0; c < n_clips; ++c) {
        clip_off[3 * c] = S.clips[c].z_off;
        clip_off[3 * c + 1] = S.clips[c].aux_off;
        clip_off[3 * c + 2] = T.clips[c].cand_off;
    }
    return PAA_OK;
}
