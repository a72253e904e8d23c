// audioSegmentation.silence_removal (audioSegmentation.py:672-815) for a batch of clips, on the device from the samples to the
// activity flags: the short-term matrices of the batched plan stay in HBM, onset_select_kernel takes the quiet and loud frames
// of every clip, onset_gather_kernel builds ONE resident training matrix and every clip's scaler, the fits of all clips are one
// batch of svc_fit_proba_resident (lib_smo.hpp), onset_weights_kernel / onset_proba_kernel score every frame with its clip's
// model and onset_threshold_kernel smooths, thresholds and flags.  Only the counts of stage 1 cross to the host before the fits
// (libsvm's folds are drawn there).  Whole clips are taken in chunks that keep the device scratch of a chunk within 1 GiB; no
// result depends on the chunking.  Kernels: kernels_onset.hpp (family_smo.hip).
#pragma once

constexpr int64_t kOnsetChunkBytes = 1LL << 30;
constexpr int kOnsetMinFrames = 20;       // int(T / 10) >= 2: both energy limits exist (ranked[-tenth:-1] is not empty)

// the device scratch a clip of T frames can need: its samples, its matrix, its per-frame arrays, its training rows (at most
// row_cap) with the solver's state over the full fit and the five fold fits
static size_t onset_clip_bytes(long long T, int n_dims, size_t sample_bytes, long long row_cap) {
    return sample_bytes + (size_t)T * ((size_t)n_dims * 8 + 19) + (size_t)row_cap * ((size_t)n_dims * 8 + 12 + 5 * 37) + 4096;
}
// [first, end) of every chunk: whole clips, as many as stay within the bound (a clip above it is a chunk of its own)
static std::vector<std::pair<int, int>> onset_chunks(const std::vector<size_t> &bytes, int64_t chunk_bytes) {
    const size_t limit = (size_t)(chunk_bytes > 0 ? std::min<int64_t>(chunk_bytes, kOnsetChunkBytes) : kOnsetChunkBytes);
    std::vector<std::pair<int, int>> chunks;
    int first = 0;
    size_t used = 0;
    for (int c = 0; c < (int)bytes.size(); ++c) {
        if (c > first && used + bytes[c] > limit) {
            chunks.push_back({first, c});
            first = c;
            used = 0;
        }
        used += bytes[c];
    }
    chunks.push_back({first, (int)bytes.size()});
    return chunks;
}

// The device arrays of a chunk: `block` holds what is known before stage 1 (per clip and per frame), `rows` what the counts of
// stage 1 size (src | alpha_y | X)
struct OnsetBuf {
    DevBlock block, rows;
    onset::OnsetDev m{};
    onset::ClipRec *d_clips = nullptr;
    double *d_rho = nullptr, *d_A = nullptr, *d_B = nullptr, *d_alpha_y = nullptr;
    int n_clips = 0, n_dims = 0;
    long long n_frames = 0, n_rows = 0;
};
static int onset_alloc(OnsetBuf &b, const double *d_feats, const std::vector<onset::ClipRec> &clips, int n_dims) {
    const size_t n = clips.size(), nf = (size_t)(clips.back().frame_off + clips.back().T);
    const size_t b_clip = up256(n * sizeof(onset::ClipRec)), b_c8 = up256(n * 8), b_c16 = up256(n * 16), b_cd = up256(n * n_dims * 8);
    const size_t b_f8 = up256(nf * 8), b_f1 = up256(nf);
    HIP_TRY(hipMalloc(&b.block.p, b_clip + 6 * b_c8 + b_c16 + 3 * b_cd + 2 * b_f8 + 3 * b_f1));
    char *p = (char *)b.block.p;
    b.d_clips = (onset::ClipRec *)p;    p += b_clip;
    b.m.limits = (double *)p;           p += b_c16;
    b.m.counts = (int *)p;              p += b_c8;
    b.m.thr = (double *)p;              p += b_c8;
    b.d_rho = (double *)p;              p += b_c8;
    b.m.intercept = (double *)p;        p += b_c8;
    b.d_A = (double *)p;                p += b_c8;
    b.d_B = (double *)p;                p += b_c8;
    b.m.mean = (double *)p;             p += b_cd;
    b.m.scale = (double *)p;            p += b_cd;
    b.m.w = (double *)p;                p += b_cd;
    b.m.raw = (double *)p;              p += b_f8;
    b.m.prob = (double *)p;             p += b_f8;
    b.m.quiet = (unsigned char *)p;     p += b_f1;
    b.m.loud = (unsigned char *)p;      p += b_f1;
    b.m.active = (unsigned char *)p;
    b.m.feats = d_feats;
    b.m.clips = b.d_clips;
    b.m.rho = b.d_rho;
    b.m.A = b.d_A;
    b.m.B = b.d_B;
    b.m.n_dims = n_dims;
    b.n_clips = (int)n;
    b.n_dims = n_dims;
    b.n_frames = (long long)nf;
    HIP_TRY(hipMemcpyAsync(b.d_clips, clips.data(), n * sizeof(onset::ClipRec), hipMemcpyHostToDevice, cs()));
    return PAA_OK;
}

// Stage 1 of a chunk: counts [n_clips][2] on the host when it returns
static int onset_select_run(OnsetBuf &b, std::vector<int32_t> &counts) {
    LAUNCH_TRY("onset selection", launch::onset_select(b.m, b.n_clips, cs()));
    counts.resize((size_t)b.n_clips * 2);
    HIP_TRY(hipMemcpyAsync(counts.data(), b.m.counts, counts.size() * 4, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}
// Stage 2 of a chunk: the counts go into the clip records with the row offsets they make, then the training matrix and scalers
static int onset_gather_run(OnsetBuf &b, std::vector<onset::ClipRec> &clips, const std::vector<int32_t> &counts) {
    long long rows = 0;
    for (int c = 0; c < b.n_clips; ++c) {
        clips[c].n_quiet = counts[2 * c];
        clips[c].n_loud = counts[2 * c + 1];
        clips[c].row_off = rows;
        rows += (long long)counts[2 * c] + counts[2 * c + 1];
    }
    b.n_rows = rows;
    const size_t r = (size_t)std::max<long long>(rows, 1), b_src = up256(r * 4), b_ay = up256(r * 8);
    HIP_TRY(hipMalloc(&b.rows.p, b_src + b_ay + r * b.n_dims * 8));
    b.m.src = (int *)b.rows.p;
    b.d_alpha_y = (double *)((char *)b.rows.p + b_src);
    b.m.alpha_y = b.d_alpha_y;
    b.m.X = (double *)((char *)b.rows.p + b_src + b_ay);
    HIP_TRY(hipMemcpyAsync(b.d_clips, clips.data(), clips.size() * sizeof(onset::ClipRec), hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));      // (the records are in pageable memory and change no more)
    LAUNCH_TRY("onset training sets", launch::onset_gather(b.m, b.n_clips, cs()));
    return PAA_OK;
}
// Stages 4 and 5 of a chunk, from the model bank w | intercept | A | B | mean | scale on the device
static int onset_activity_run(OnsetBuf &b) {
    LAUNCH_TRY("onset probability", launch::onset_proba(b.m, b.n_clips, b.n_frames, cs()));
    LAUNCH_TRY("onset threshold", launch::onset_threshold(b.m, b.n_clips, cs()));
    return PAA_OK;
}

// what the stage entry points ask of a list of short-term matrices
static int onset_frames_check(const int32_t *frames, int n_clips, int n_dims) {
    if (n_clips < 1) return fail(PAA_ERR_ARG, "no clips");
    if (n_dims < 2 || n_dims > onset::kMaxDims) return fail(PAA_ERR_ARG, "%d feature rows: 2 .. %d (row 1 is the energy)", n_dims, onset::kMaxDims);
    for (int c = 0; c < n_clips; ++c)
        if (frames[c] < kOnsetMinFrames) return fail(PAA_ERR_ARG, "clip %d: %d frames: at least %d are needed", c, frames[c], kOnsetMinFrames);
    return PAA_OK;
}
// the clip records of the chunk [c0, c1) of matrices that lie back to back, and the first double of the chunk
static std::vector<onset::ClipRec> onset_chunk_clips(const int32_t *frames, int c0, int c1, int n_dims, const int32_t *widths,
                                                     const double *weights) {
    std::vector<onset::ClipRec> clips((size_t)(c1 - c0));
    long long feat = 0, frame = 0;
    for (int c = c0; c < c1; ++c) {
        onset::ClipRec &r = clips[(size_t)(c - c0)];
        r = onset::ClipRec{feat, frame, 0, frames[c], 0, 0, widths ? widths[c] : 0, weights ? weights[c] : 0.5};
        feat += (long long)n_dims * frames[c];
        frame += frames[c];
    }
    return clips;
}

// Stages 1 and 2 for short-term matrices in host memory: see paa_hip.h
extern "C" int paa_onset_training_sets_f64(const double *feats, const int32_t *frames, int n_clips, int n_dims, int64_t chunk_bytes,
                                           int64_t row_capacity, double *limits, int32_t *counts, uint8_t *quiet, uint8_t *loud,
                                           int32_t *src, double *X, double *mean, double *scale) {
    if (!feats || !frames || !limits || !counts || !quiet || !loud || !src || !X || !mean || !scale) return fail(PAA_ERR_ARG, "null argument");
    int rc;
    if ((rc = onset_frames_check(frames, n_clips, n_dims))) return rc;
    if ((rc = ensure_init())) return rc;
    LaneGuard lane;
    std::vector<size_t> bytes((size_t)n_clips);
    for (int c = 0; c < n_clips; ++c) bytes[c] = onset_clip_bytes(frames[c], n_dims, 0, 2LL * frames[c]);
    long long feat0 = 0, frame0 = 0, row0 = 0;
    for (const auto &ch : onset_chunks(bytes, chunk_bytes)) {
        std::vector<onset::ClipRec> clips = onset_chunk_clips(frames, ch.first, ch.second, n_dims, nullptr, nullptr);
        const int n = ch.second - ch.first;
        const long long nd = clips.back().feat_off + (long long)n_dims * clips.back().T, nf = clips.back().frame_off + clips.back().T;
        {
            std::lock_guard<std::mutex> lk(g_mu);
            if ((rc = scratch_reserve(lane.l->in, (size_t)nd * 8))) return rc;
        }
        HIP_TRY(hipMemcpyAsync(lane.l->in.p, feats + feat0, (size_t)nd * 8, hipMemcpyHostToDevice, cs()));
        OnsetBuf b;
        std::vector<int32_t> cnt;
        if ((rc = onset_alloc(b, (const double *)lane.l->in.p, clips, n_dims))) return rc;
        if ((rc = onset_select_run(b, cnt))) return rc;
        if ((rc = onset_gather_run(b, clips, cnt))) return rc;
        if (row0 + b.n_rows > row_capacity)
            return fail(PAA_ERR_ARG, "row_capacity = %lld: the clips up to %d make %lld training rows", (long long)row_capacity, ch.second - 1, row0 + b.n_rows);
        std::copy(cnt.begin(), cnt.end(), counts + 2 * (size_t)ch.first);
        HIP_TRY(hipMemcpyAsync(limits + 2 * (size_t)ch.first, b.m.limits, (size_t)n * 16, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(quiet + frame0, b.m.quiet, (size_t)nf, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(loud + frame0, b.m.loud, (size_t)nf, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(mean + (size_t)ch.first * n_dims, b.m.mean, (size_t)n * n_dims * 8, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(scale + (size_t)ch.first * n_dims, b.m.scale, (size_t)n * n_dims * 8, hipMemcpyDeviceToHost, cs()));
        if (b.n_rows) {
            HIP_TRY(hipMemcpyAsync(src + row0, b.m.src, (size_t)b.n_rows * 4, hipMemcpyDeviceToHost, cs()));
            HIP_TRY(hipMemcpyAsync(X + row0 * n_dims, b.m.X, (size_t)b.n_rows * n_dims * 8, hipMemcpyDeviceToHost, cs()));
        }
        HIP_TRY(hipStreamSynchronize(cs()));
        feat0 += nd;
        frame0 += nf;
        row0 += b.n_rows;
    }
    return PAA_OK;
}

// Stages 4 and 5 for short-term matrices and linear models in host memory: see paa_hip.h
extern "C" int paa_onset_activity_f64(const double *feats, const int32_t *frames, int n_clips, int n_dims, const double *w,
                                      const double *intercept, const double *prob_a, const double *prob_b, const double *mean,
                                      const double *scale, const int32_t *widths, const double *weights, int64_t chunk_bytes,
                                      double *raw, double *prob, double *threshold, uint8_t *active) {
    if (!feats || !frames || !w || !intercept || !prob_a || !prob_b || !mean || !scale || !widths || !weights || !raw || !prob || !threshold || !active)
        return fail(PAA_ERR_ARG, "null argument");
    int rc;
    if ((rc = onset_frames_check(frames, n_clips, n_dims))) return rc;
    for (int c = 0; c < n_clips; ++c)
        if (widths[c] > frames[c]) return fail(PAA_ERR_ARG, "clip %d: Input vector needs to be bigger than window size (%d frames, a window of %d)", c, frames[c], widths[c]);
    if ((rc = ensure_init())) return rc;
    LaneGuard lane;
    std::vector<size_t> bytes((size_t)n_clips);
    for (int c = 0; c < n_clips; ++c) bytes[c] = onset_clip_bytes(frames[c], n_dims, 0, 0);
    long long feat0 = 0, frame0 = 0;
    for (const auto &ch : onset_chunks(bytes, chunk_bytes)) {
        const std::vector<onset::ClipRec> clips = onset_chunk_clips(frames, ch.first, ch.second, n_dims, widths, weights);
        const size_t n = (size_t)(ch.second - ch.first), c0 = (size_t)ch.first, sb = n * n_dims * 8;
        const long long nd = clips.back().feat_off + (long long)n_dims * clips.back().T, nf = clips.back().frame_off + clips.back().T;
        {
            std::lock_guard<std::mutex> lk(g_mu);
            if ((rc = scratch_reserve(lane.l->in, (size_t)nd * 8))) return rc;
        }
        HIP_TRY(hipMemcpyAsync(lane.l->in.p, feats + feat0, (size_t)nd * 8, hipMemcpyHostToDevice, cs()));
        OnsetBuf b;
        if ((rc = onset_alloc(b, (const double *)lane.l->in.p, clips, n_dims))) return rc;
        HIP_TRY(hipMemcpyAsync(b.m.w, w + c0 * n_dims, sb, hipMemcpyHostToDevice, cs()));
        HIP_TRY(hipMemcpyAsync(b.m.mean, mean + c0 * n_dims, sb, hipMemcpyHostToDevice, cs()));
        HIP_TRY(hipMemcpyAsync(b.m.scale, scale + c0 * n_dims, sb, hipMemcpyHostToDevice, cs()));
        HIP_TRY(hipMemcpyAsync(b.m.intercept, intercept + c0, n * 8, hipMemcpyHostToDevice, cs()));
        HIP_TRY(hipMemcpyAsync(b.d_A, prob_a + c0, n * 8, hipMemcpyHostToDevice, cs()));
        HIP_TRY(hipMemcpyAsync(b.d_B, prob_b + c0, n * 8, hipMemcpyHostToDevice, cs()));
        if ((rc = onset_activity_run(b))) return rc;
        HIP_TRY(hipMemcpyAsync(raw + frame0, b.m.raw, (size_t)nf * 8, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(prob + frame0, b.m.prob, (size_t)nf * 8, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(active + frame0, b.m.active, (size_t)nf, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipMemcpyAsync(threshold + c0, b.m.thr, n * 8, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipStreamSynchronize(cs()));
        feat0 += nd;
        frame0 += nf;
    }
    return PAA_OK;
}

// ---- the whole chain ------------------------------------------------------------------------------------------------------------

// host arrays of paa_silence_batch_*: per frame, per clip and per training row (a clip's rows begin at row_cap_off [clip])
struct SilenceOut {
    uint8_t *quiet, *loud, *active;
    double *raw, *prob;
    double *limits;
    int32_t *counts;
    double *mean, *scale;
    int32_t *src;
    double *alpha_y, *rho, *prob_a, *prob_b, *threshold;
    int32_t *n_sv, *iterations, *status, *sig_iterations, *sig_stop;
    double *stage_ms;         // [6] or null: features, selection, training sets, fits, probability and threshold, copy-back
    int32_t *clip_cached = nullptr;       // [n_clips], paa_silence_batch_*_cached: the clip's fits read a resident kernel matrix under the
    int64_t cache_bytes = 0;              // budget cache_bytes (null: no resident matrices)
};

struct StageClock {
    double *ms;
    std::chrono::steady_clock::time_point t0;
    explicit StageClock(double *out) : ms(out), t0(std::chrono::steady_clock::now()) {}
    // the time since the previous mark goes to `stage`; the stream is drained first, and only when times are wanted
    int mark(int stage) {
        if (!ms) return PAA_OK;
        HIP_TRY(hipStreamSynchronize(cs()));
        const auto t1 = std::chrono::steady_clock::now();
        ms[stage] += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return PAA_OK;
    }
};

// One chunk [c0, c1) of the batch.  select_only: stop after the checks that follow stage 1 (the first pass of a batch of
// several chunks, so that no fit starts before every clip's counts are known to be usable)
static int silence_chunk(Lane &lane, const void *packed, const int64_t *offsets, int c0, int c1, int sample_kind, double fs, int window,
                         int step, const std::vector<int64_t> &frame_off, const int32_t *widths, const double *weights,
                         const int64_t *seeds, const int64_t *row_cap_off, bool select_only, const SilenceOut &o) {
    const int n = c1 - c0, n_dims = 2 * kBase;
    const size_t esz = sample_kind == 0 ? 2 : 8;
    StageClock clock(o.stage_ms);
    int rc;
    // the host vectors that asynchronous copies read or fill, and behind them the guard that drains the stream on EVERY return: it
    // goes first, so no copy is in flight when an error path lets the vectors go
    std::vector<onset::ClipRec> clips((size_t)n);
    std::vector<int32_t> cnt, src;
    std::vector<double> alpha_y;
    struct Drain { ~Drain() { (void)hipStreamSynchronize(cs()); } } drain;
    // the short-term matrices of the chunk: [n_dims][T] blocks in the lane's out scratch
    std::vector<int64_t> off((size_t)n + 1);
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
        if ((rc = scratch_reserve(lane.in, (size_t)off[n] * esz + 64))) return rc;
        if ((rc = scratch_reserve(lane.out, (size_t)plan->out_doubles * 8))) return rc;
    }
    HIP_TRY(hipMemcpyAsync(lane.in.p, (const char *)packed + (size_t)offsets[c0] * esz, (size_t)off[n] * esz, hipMemcpyHostToDevice, cs()));
    if ((rc = paa_plan_execute(plan, lane.in.p, (double *)lane.out.p))) return rc;
    if ((rc = clock.mark(0))) return rc;
    // stage 1
    for (int c = 0; c < n; ++c) {
        const int64_t T = frame_off[c0 + c + 1] - frame_off[c0 + c];
        if (plan->clips[c].T != T) return fail(PAA_ERR_ARG, "clip %d: %d frames in the plan, %lld expected", c0 + c, plan->clips[c].T, (long long)T);
        clips[c] = onset::ClipRec{plan->clips[c].out_off, frame_off[c0 + c] - frame_off[c0], 0, (int)T, 0, 0, widths[c0 + c], weights[c0 + c]};
    }
    OnsetBuf b;
    if ((rc = onset_alloc(b, (const double *)lane.out.p, clips, n_dims))) return rc;
    if ((rc = onset_select_run(b, cnt))) return rc;
    if ((rc = clock.mark(1))) return rc;
    for (int c = 0; c < n; ++c) {
        const long long rows = (long long)cnt[2 * c] + cnt[2 * c + 1];
        if (cnt[2 * c] < 1 || cnt[2 * c + 1] < 1)
            return fail(PAA_ERR_ARG, "clip %d: %d quiet and %d loud frames: the number of classes has to be greater than one", c0 + c, cnt[2 * c], cnt[2 * c + 1]);
        if (rows > smo::kMaxRows)
            return fail(PAA_ERR_UNSUPPORTED, "clip %d: %lld quiet + loud rows: the GPU solver serves at most %d rows per fit", c0 + c, rows, smo::kMaxRows);
        if (rows > row_cap_off[c0 + c + 1] - row_cap_off[c0 + c])
            return fail(PAA_ERR_ARG, "clip %d: %lld training rows, room for %lld", c0 + c, rows, (long long)(row_cap_off[c0 + c + 1] - row_cap_off[c0 + c]));
    }
    if (select_only) return PAA_OK;
    // stage 2
    if ((rc = onset_gather_run(b, clips, cnt))) return rc;
    if ((rc = clock.mark(2))) return rc;
    // stage 3: one job per clip over its rows (the quiet rows class 0, the loud rows class 1), C = 1, linear, gamma = 1 / n_dims
    const size_t rows = (size_t)b.n_rows;
    std::vector<int32_t> labels(rows), train_idx(rows);
    std::vector<int64_t> train_off((size_t)n + 1);
    for (int c = 0; c < n; ++c) {
        train_off[c] = clips[c].row_off;
        std::fill(labels.begin() + clips[c].row_off, labels.begin() + clips[c].row_off + clips[c].n_quiet, 0);
        std::fill(labels.begin() + clips[c].row_off + clips[c].n_quiet, labels.begin() + clips[c].row_off + clips[c].n_quiet + clips[c].n_loud, 1);
    }
    train_off[n] = (int64_t)rows;
    for (size_t i = 0; i < rows; ++i) train_idx[i] = (int32_t)i;
    const std::vector<double> C_one((size_t)n, 1.0), gamma((size_t)n, 1.0 / n_dims);
    PairTasks p;
    if ((rc = svc_pair_tasks(p, labels.data(), n, train_off.data(), train_idx.data(), C_one.data(), gamma.data(), 0))) return rc;
    alpha_y.resize(rows);
    const ProbaFitOut fit{alpha_y.data(), o.rho + c0, o.prob_a + c0, o.prob_b + c0, o.n_sv + c0, o.iterations + 6 * (size_t)c0,
                          o.status + 6 * (size_t)c0, o.sig_iterations + c0, o.sig_stop + c0, nullptr, nullptr,
                          o.clip_cached ? o.clip_cached + c0 : nullptr, o.cache_bytes};
    if ((rc = svc_fit_proba_resident(b.m.X, b.m.mean, b.m.scale, n_dims, p, seeds + c0, 0, 1e-3, 10000000, 0, fit))) return rc;
    if ((rc = clock.mark(3))) return rc;
    // stages 4 and 5
    HIP_TRY(hipMemcpyAsync(b.d_alpha_y, alpha_y.data(), rows * 8, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemcpyAsync(b.d_rho, o.rho + c0, (size_t)n * 8, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemcpyAsync(b.d_A, o.prob_a + c0, (size_t)n * 8, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipMemcpyAsync(b.d_B, o.prob_b + c0, (size_t)n * 8, hipMemcpyHostToDevice, cs()));
    LAUNCH_TRY("onset weights", launch::onset_weights(b.m, n, cs()));
    if ((rc = onset_activity_run(b))) return rc;
    if ((rc = clock.mark(4))) return rc;
    // copy back
    const size_t f0 = (size_t)frame_off[c0], nf = (size_t)b.n_frames;
    src.resize(rows);
    HIP_TRY(hipMemcpyAsync(o.quiet + f0, b.m.quiet, nf, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(o.loud + f0, b.m.loud, nf, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(o.active + f0, b.m.active, nf, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(o.raw + f0, b.m.raw, nf * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(o.prob + f0, b.m.prob, nf * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(o.limits + 2 * (size_t)c0, b.m.limits, (size_t)n * 16, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(o.mean + (size_t)c0 * n_dims, b.m.mean, (size_t)n * n_dims * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(o.scale + (size_t)c0 * n_dims, b.m.scale, (size_t)n * n_dims * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(o.threshold + c0, b.m.thr, (size_t)n * 8, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipMemcpyAsync(src.data(), b.m.src, rows * 4, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    std::copy(cnt.begin(), cnt.end(), o.counts + 2 * (size_t)c0);
    for (int c = 0; c < n; ++c) {
        const size_t r0 = (size_t)clips[c].row_off, r1 = r0 + (size_t)clips[c].n_quiet + (size_t)clips[c].n_loud;
        std::copy(src.begin() + r0, src.begin() + r1, o.src + row_cap_off[c0 + c]);
        std::copy(alpha_y.begin() + r0, alpha_y.begin() + r1, o.alpha_y + row_cap_off[c0 + c]);
    }
    return clock.mark(5);
}

static int run_silence_batch(const void *packed, const int64_t *offsets, int64_t n_clips, int sample_kind, double fs, int window, int step,
                             const int32_t *widths, const double *weights, const int64_t *seeds, int64_t chunk_bytes,
                             const int64_t *row_cap_off, const SilenceOut &o) {
    if (!packed || !offsets || !widths || !weights || !seeds || !row_cap_off || !o.quiet || !o.loud || !o.active || !o.raw || !o.prob ||
        !o.limits || !o.counts || !o.mean || !o.scale || !o.src || !o.alpha_y || !o.rho || !o.prob_a || !o.prob_b || !o.threshold ||
        !o.n_sv || !o.iterations || !o.status || !o.sig_iterations || !o.sig_stop)
        return fail(PAA_ERR_ARG, "null argument");
    if (o.clip_cached && o.cache_bytes <= 0) return fail(PAA_ERR_ARG, "cache_bytes = %lld: a positive budget is needed", (long long)o.cache_bytes);
    if (n_clips < 1 || n_clips > 0x3fffffffLL) return fail(PAA_ERR_ARG, "%lld clips", (long long)n_clips);
    if (window < 2 || step < 1) return fail(PAA_ERR_ARG, "window=%d step=%d: need window >= 2, step >= 1", window, step);
    const int n_dims = 2 * kBase;
    const size_t esz = sample_kind == 0 ? 2 : 8;
    std::vector<int64_t> frame_off((size_t)n_clips + 1, 0);
    std::vector<size_t> bytes((size_t)n_clips);
    for (int64_t c = 0; c < n_clips; ++c) {
        const int64_t len = offsets[c + 1] - offsets[c], T = len >= 0 ? paa_num_frames(len, window, step) : 0;
        if (T < kOnsetMinFrames)
            return fail(PAA_ERR_ARG, "clip %lld: %lld frames: at least %d are needed (a tenth of them is averaged without its maximum)", (long long)c, (long long)T, kOnsetMinFrames);
        if (T > 0x7fffffffLL) return fail(PAA_ERR_ARG, "clip %lld has too many frames", (long long)c);
        if (widths[c] > T)
            return fail(PAA_ERR_ARG, "clip %lld: Input vector needs to be bigger than window size (%lld frames, a window of %d)", (long long)c, (long long)T, widths[c]);
        if (seeds[c] < 0 || seeds[c] > 0x7fffffffLL) return fail(PAA_ERR_ARG, "clip %lld: seed %lld: libsvm's random_seed is in 0 .. 2^31 - 1", (long long)c, (long long)seeds[c]);
        frame_off[c + 1] = frame_off[c] + T;
        bytes[c] = onset_clip_bytes(T, n_dims, (size_t)len * esz, std::min<long long>(2 * T, smo::kMaxRows));
    }
    int rc;
    if ((rc = ensure_init())) return rc;
    LaneGuard lane;       // own stream + scratch for this call (see Lane)
    if (o.stage_ms) std::fill(o.stage_ms, o.stage_ms + 6, 0.0);
    const std::vector<std::pair<int, int>> chunks = onset_chunks(bytes, chunk_bytes);
    if (chunks.size() > 1) {
        SilenceOut first_pass = o;
        first_pass.stage_ms = nullptr;
        for (const auto &ch : chunks)
            if ((rc = silence_chunk(*lane.l, packed, offsets, ch.first, ch.second, sample_kind, fs, window, step, frame_off, widths, weights,
                                    seeds, row_cap_off, true, first_pass)))
                return rc;
    }
    for (const auto &ch : chunks)
        if ((rc = silence_chunk(*lane.l, packed, offsets, ch.first, ch.second, sample_kind, fs, window, step, frame_off, widths, weights, seeds,
                                row_cap_off, false, o)))
            return rc;
    return PAA_OK;
}

#define PAA_SILENCE_BATCH_ARGS                                                                                                            \
    const int64_t *offsets, int64_t n_clips, double fs, int window, int step, const int32_t *widths, const double *weights,               \
        const int64_t *seeds, int64_t chunk_bytes, const int64_t *row_cap_off, uint8_t *quiet, uint8_t *loud, uint8_t *active, double *raw, \
        double *prob, double *limits, int32_t *counts, double *mean, double *scale, int32_t *src, double *alpha_y, double *rho,           \
        double *prob_a, double *prob_b, double *threshold, int32_t *n_sv, int32_t *iterations, int32_t *status, int32_t *sig_iterations,  \
        int32_t *sig_stop, double *stage_ms
#define PAA_SILENCE_BATCH_OUT                                                                                                             \
    SilenceOut { quiet, loud, active, raw, prob, limits, counts, mean, scale, src, alpha_y, rho, prob_a, prob_b, threshold, n_sv,         \
                 iterations, status, sig_iterations, sig_stop, stage_ms }

// silence_removal for a batch of clips: see paa_hip.h
extern "C" int paa_silence_batch_i16(const int16_t *packed, PAA_SILENCE_BATCH_ARGS) {
    return run_silence_batch(packed, offsets, n_clips, 0, fs, window, step, widths, weights, seeds, chunk_bytes, row_cap_off, PAA_SILENCE_BATCH_OUT);
}
extern "C" int paa_silence_batch_f64(const double *packed, PAA_SILENCE_BATCH_ARGS) {
    return run_silence_batch(packed, offsets, n_clips, 1, fs, window, step, widths, weights, seeds, chunk_bytes, row_cap_off, PAA_SILENCE_BATCH_OUT);
}
// ... with every clip's full fit and fold fits on one resident kernel matrix (paa_svc_fit_proba_cached_f64's form: a clip is a job)
static int run_silence_batch_cached(const void *packed, const int64_t *offsets, int64_t n_clips, int sample_kind, double fs, int window,
                                    int step, const int32_t *widths, const double *weights, const int64_t *seeds, int64_t chunk_bytes,
                                    const int64_t *row_cap_off, SilenceOut o, int64_t cache_bytes, int32_t *clip_cached) {
    if (!clip_cached) return fail(PAA_ERR_ARG, "null argument");
    o.clip_cached = clip_cached;
    o.cache_bytes = cache_bytes;
    return run_silence_batch(packed, offsets, n_clips, sample_kind, fs, window, step, widths, weights, seeds, chunk_bytes, row_cap_off, o);
}
extern "C" int paa_silence_batch_i16_cached(const int16_t *packed, PAA_SILENCE_BATCH_ARGS, int64_t cache_bytes, int32_t *clip_cached) {
    return run_silence_batch_cached(packed, offsets, n_clips, 0, fs, window, step, widths, weights, seeds, chunk_bytes, row_cap_off,
                                    PAA_SILENCE_BATCH_OUT, cache_bytes, clip_cached);
}
extern "C" int paa_silence_batch_f64_cached(const double *packed, PAA_SILENCE_BATCH_ARGS, int64_t cache_bytes, int32_t *clip_cached) {
    return run_silence_batch_cached(packed, offsets, n_clips, 1, fs, window, step, widths, weights, seeds, chunk_bytes, row_cap_off,
                                    PAA_SILENCE_BATCH_OUT, cache_bytes, clip_cached);
}
#undef PAA_SILENCE_BATCH_ARGS
#undef PAA_SILENCE_BATCH_OUT
