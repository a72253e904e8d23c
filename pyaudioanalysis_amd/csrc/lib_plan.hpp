// Plans: clip descriptors, statistics chunks, run lengths and tile lists, the kernel choice (lib_dispatch.hpp) and the
// device-resident plan API (paa_plan_create / _execute / _mid_execute / _beat_execute ...).  One of the units paa_lib.hip is
// made of (included there, after the library state; not a translation unit of its own).
#pragma once
// ------------------------------------------------------------------------------------------
// plans
// ------------------------------------------------------------------------------------------
#ifndef PAA_STAT_CHUNK
#define PAA_STAT_CHUNK 131072         // (A/B of scripts/rounds/r05/gpu_r05aj.sh against 65536: two workgroups per CU for the one-hour clip instead of
                                      // four leave the pass at 20.4 us and halve the partials every wave of the feature kernel folds
                                      // in its prologue: 259.9 -> 258.5 us.  int32 partial sums: 512 samples of |v| < 2^16 per thread)
#endif
constexpr int kStatChunk = PAA_STAT_CHUNK;          // samples per statistics workgroup (upper bound, see stat_chunk_for)
// The statistics pass is an HBM-bound stream with every workgroup resident at once (8 per CU): 879 chunks of 64 K samples of a
// one-hour clip put 4 workgroups on some CUs and 3 on others, and the pass lasts as long as the CUs with 4.  A batch of at least
// one chunk per CU is therefore cut into a whole multiple of num_cu chunks (512 x 112 512 samples for the hour).
static int stat_chunk_for(long long total_samples, int num_cu) {
    const long long blocks = (total_samples + kStatChunk - 1) / kStatChunk;
    if (blocks < num_cu) {
        // a short batch (one 60 s stereo clip = 41 chunks of 64 K) left 215 CUs idle and each workgroup with sixteen dependent
        // rounds of loads: 16.7 us for 10.6 MB.  Four chunks per CU of at least 4096 samples (one round of loads) instead.
        const long long len = ((total_samples + 4LL * num_cu - 1) / (4LL * num_cu) + 63) / 64 * 64;
        return (int)std::min<long long>(kStatChunk, std::max<long long>(len, 4096));
    }
    const long long want = (blocks + num_cu - 1) / num_cu * num_cu;
    const long long len = ((total_samples + want - 1) / want + 63) / 64 * 64;      // multiples of 64 samples keep the 16-byte body aligned
    return (int)std::min<long long>(kStatChunk, std::max<long long>(len, 4096));
}

// Run length for the one-wave-per-run kernels.  A clip of T frames is cut into k = ceil(T / cap) runs of
// len = ceil(T / k) frames rounded up to the kernel's quantum (so no clip ends in a short leftover run); a workgroup takes
// wg_runs consecutive runs and the chip holds num_cu workgroups at a time, so a launch lasts about
// ceil(workgroups / num_cu) rounds of (longest run + halo) frames.  The cap that minimises that estimate is returned:
// one 1-hour clip -> 2000 runs of 72 frames (one round); 12 500 clips of 399 frames -> two runs of 200 per clip instead
// of 244 + 155 (the short run's wave idled for a third of its workgroup's life); 1000 clips of 1199 frames -> 6 x 200.
static int choose_run_cap(const std::vector<ClipDev> &clips, int quantum, int min_run, int max_run, int halo, int wg_runs,
                          int num_cu, int shrink = 0) {
    // shrink: frames by which every run but a clip's first is shorter (kernels whose halo rides inside the first iteration:
    // the tile list gives those runs len - shrink frames, so a clip has more runs than T / len)
    std::map<long long, long long> hist;                       // frames per clip -> number of such clips
    for (const ClipDev &c : clips)
        if (c.T > 0) ++hist[c.T];
    if (hist.empty()) return max_run;
    long long best_cost = -1;
    int best = max_run;
    for (int cap = max_run / quantum * quantum; cap >= min_run; cap -= quantum) {
        long long runs = 0, longest = 0;
        for (const auto &kv : hist) {
            const long long k = (kv.first + cap - 1) / cap;
            const long long len = ((kv.first + k - 1) / k + quantum - 1) / quantum * quantum;
            const long long later = std::max<long long>(len - shrink, 1);
            runs += kv.second * ((kv.first <= len) ? 1 : 1 + (kv.first - len + later - 1) / later);
            longest = std::max(longest, len);
        }
        const long long wgs = (runs + wg_runs - 1) / wg_runs;
        const long long rounds = (wgs + num_cu - 1) / num_cu;
        const long long cost = rounds * (longest + halo);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = cap; }     // ties: the longer run (fewer halos)
    }
    return best;
}
// the runs of one clip of T frames under a cap: k = ceil(T / cap) runs of ceil(T / k) frames, rounded up to the quantum
static inline int clip_run_length(long long T, int cap, int quantum) {
    const long long k = (T + cap - 1) / cap;
    return (int)(((T + k - 1) / k + quantum - 1) / quantum * quantum);
}

// Run lengths of a plan that fills LESS than one round of a one-workgroup-per-CU kernel (the one-hour clip: 2000 equal runs of
// 72 frames = 250 workgroups of eight on 256 CUs, scripts/experiments/run_geometry.py: 256 workgroups take the same time).  Every
// clip is re-cut into its share of num_cu x wg_runs runs whose ITERATION counts (quanta) differ by at most one; runs after a
// clip's first hold `shrink` halo frames inside their first iteration, i.e. store that many frames less.  Along the order
// (workgroup, SIMD, wave of the SIMD) long and short runs alternate, so the waves that share a SIMD (w, w + 4, ...) get long and
// short ones in the plan's overall ratio.  Returns false (lens untouched) when the equal runs stay.
// xcd_order (optional; eight labels, label = workgroup mod 8, the slowest XCD's first -- lib_xcd_order.hpp): a launch lasts as long as
// its slowest XCD needs for its largest SIMD total, so the SHORT runs go where they shorten that: a clip keeps its numbers of long
// and short runs, but the shorts are dealt one per SIMD group (the `per` waves of a SIMD), label after label in the given order,
// workgroup after workgroup inside a label, and only then a second one per group.  Inside a group the member the even spread
// makes short is taken first, then the last one.  Without an order (or a permutation, or a chip of num_cu % 8 workgroups more,
// or waves that do not pair up on the SIMDs) the even spread stays, byte for byte.
static bool balanced_runs(const std::vector<ClipDev> &clips, int run, int quantum, int shrink, int wg_runs, int num_cu, int min_run,
                          std::vector<std::vector<int>> &lens, const int *xcd_order = nullptr) {
    if (wg_runs < 2 || quantum < 1 || shrink < 0 || (shrink > 0 && shrink >= quantum)) return false;
    int rank[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (xcd_order) {
        int seen = 0;
        for (int r = 0; r < 8; ++r)
            if (xcd_order[r] >= 0 && xcd_order[r] < 8) { rank[xcd_order[r]] = r; seen |= 1 << xcd_order[r]; }
        if (seen != 0xff || num_cu % 8 != 0 || wg_runs % 4 != 0) xcd_order = nullptr;
    }
    long long total = 0, runs = 0;
    std::vector<long long> need(clips.size(), 0);
    for (size_t c = 0; c < clips.size(); ++c) {
        const long long T = clips[c].T;
        if (T <= 0) continue;
        total += T;
        const long long len = clip_run_length(T, run, quantum), later = std::max<long long>(len - shrink, 1);
        need[c] = (T <= len) ? 1 : 1 + (T - len + later - 1) / later;          // the tile rule of the equal runs
        runs += need[c];
    }
    const long long slots = (long long)num_cu * wg_runs;
    if (runs >= slots || (runs + wg_runs - 1) / wg_runs > num_cu || total < slots * min_run) return false;
    // runs per clip: proportional to its frames (at least what the cap asks for), never shorter than min_run frames
    std::vector<long long> k(clips.size(), 0);
    long long given = 0;
    for (size_t c = 0; c < clips.size(); ++c) {
        const long long T = clips[c].T;
        if (T <= 0) continue;
        k[c] = std::max<long long>(need[c], std::min<long long>(slots * T / total, std::max<long long>(T / min_run, 1)));
        given += k[c];
    }
    if (given > slots) return false;
    std::vector<std::vector<int>> out(clips.size());
    // waves w, w + 4, w + 8 ... of a workgroup share a SIMD (profiles/r05_fast800_wave_trace.txt): per = waves per SIMD
    const int per = (wg_runs % 4 == 0) ? wg_runs / 4 : 0;
    long long first_tile = 0;          // tile index of the clip's first run (runs of all clips are laid out consecutively)
    for (size_t c = 0; c < clips.size(); ++c) {
        const long long T = clips[c].T, kc = k[c];
        if (T <= 0) continue;
        const long long iters = (T + (kc - 1) * shrink + quantum - 1) / quantum, base = iters / kc, longs = iters % kc;
        if (base < 1 || (base + (longs ? 1 : 0)) * quantum > run) return false;
        std::vector<int> &l = out[c];
        l.assign((size_t)kc, (int)(base * quantum));
        // position u of the (workgroup, SIMD, member) order -> run; `longs` of the kc positions get one more iteration, spread evenly
        std::vector<std::pair<long long, long long>> order;
        order.reserve((size_t)kc);
        for (long long i = 0; i < kc; ++i) {
            const long long tile = first_tile + i, w = tile % wg_runs, j = tile / wg_runs;
            order.emplace_back(per ? (j * 4 + w % 4) * per + w / 4 : tile, i);
        }
        std::sort(order.begin(), order.end());
        std::vector<char> is_long((size_t)kc, 0);          // by position u
        for (long long u = 0; u < kc; ++u) is_long[(size_t)u] = (u + 1) * longs / kc > u * longs / kc;
        if (xcd_order && longs > 0) {
            struct Group { long long key, u0; int n, given; };          // key: (rank of the label, workgroup, SIMD); positions [u0, u0 + n)
            std::vector<Group> groups;
            for (long long u = 0; u < kc; ++u) {
                const long long gid = order[(size_t)u].first / per, j = gid / 4;
                const long long key = ((long long)rank[j % 8] << 40) | gid;
                if (groups.empty() || groups.back().key != key) groups.push_back(Group{key, u, 0, 0});
                ++groups.back().n;
            }
            std::sort(groups.begin(), groups.end(), [](const Group &a, const Group &b) { return a.key < b.key; });
            const std::vector<char> even = is_long;
            std::fill(is_long.begin(), is_long.end(), 1);
            for (long long left = kc - longs; left > 0;)
                for (Group &g : groups) {          // one round: a short run more for every group that still has a long one
                    if (left == 0) break;
                    if (g.given == g.n) continue;
                    long long pick = -1;
                    for (long long u = g.u0 + g.n - 1; u >= g.u0; --u)
                        if (is_long[(size_t)u] && (pick < 0 || (!even[(size_t)u] && even[(size_t)pick]))) pick = u;
                    is_long[(size_t)pick] = 0;
                    ++g.given;
                    --left;
                }
        }
        for (long long u = 0; u < kc; ++u)
            if (is_long[(size_t)u]) l[(size_t)order[(size_t)u].second] += quantum;
        long long sum = 0;
        for (size_t i = 0; i < l.size(); ++i) { if (i > 0) l[i] -= shrink; sum += l[i]; }
        l.back() -= (int)(sum - T);          // the iterations cover whole quanta: the last run gives back what the clip does not have
        if (l.back() <= 0) return false;
        first_tile += kc;
    }
    lens.swap(out);
    return true;
}

#include "lib_xcd_order.hpp"

// the kernel choice of a plan: its entry of kFamilies (lib_dispatch.hpp), the layout of that entry's kernel (only its own member
// is meaningful) and the table blob on the device.  Cached per (table set, mode, rows) in TableSet::choices.
struct FamilyChoice {
    int family = -1;                 // index into kFamilies
    FastLaunch fl;                   // kernels_fast.hpp
    ct::CtLaunch cl;                 // kernels_ct.hpp
    tri::TriLaunch trl;              // kernels_tri.hpp
    mix::MixLayout ml;               // kernels_mix.hpp
    blu::BluLayout bl;               // kernels_blu.hpp
    GenLayout gl;                    // kernels_generic.hpp
    wg::WgLayout wl;                 // kernels_wg.hpp: r0 = 0 runs on run_wg_lds, r0 > 0 on run_wg_split (kernels_wgs.hpp: r0 > 0 is its select's
                                     // condition; its own (r0, q) come from wgs_select)
    size_t lds = 0;
    std::string kernel_name;
    unsigned char *d_blob = nullptr;       // the entry's device tables (ct, tri, mix, blu, generic: LDS + global tables; wgr: WgrTab;
                                           // wg: the digit-reversal permutation), or none
};

struct paa_plan {
    long long n_clips = 0;
    int sample_kind = 0;
    int mode = 0;                   // 0 features, 1 spectrogram, 2 chromagram
    int row_width = 0;              // doubles per frame of the slab in modes 1/2
    std::vector<ClipDev> clips;
    std::vector<long long> alloc_rows;   // modes 1/2: rows the reference allocates per clip
    long long total_frames = 0, out_doubles = 0;
    TableSet *tab = nullptr;
    int stat_chunk = kStatChunk;     // samples per statistics chunk of this plan
    PlanDev P;
    ClipDev *d_clips = nullptr;
    ClipNorm *d_norms = nullptr;
    Tile *d_tiles = nullptr;
    StatChunk *d_chunks = nullptr;
    void *d_psum = nullptr, *d_pmin = nullptr, *d_pmax = nullptr;
    long long *d_mid_off = nullptr;
    FamilyChoice fam;                // the kernel that runs the plan (lib_dispatch.hpp)
    bool blob_cached = false;        // fam.d_blob belongs to the table set's cached FamilyChoice (not freed with the plan)
    void *d_block = nullptr;         // the plan's one device block: d_clips, d_tiles, d_chunks, d_norms, d_psum / pmin / pmax point into it
    void *d_big = nullptr;           // scratch of the big-window paths (grow_big; wg_scratch carves it for run_wg_lds / run_wg_split / run_wgs, run_big for itself)
    size_t big_bytes = 0;
    std::vector<wg::FrameRef> wg_frames;              // every frame of the plan, chunk after chunk (a chunk's rows fit the scratch)
    std::vector<std::pair<long long, long long>> wg_chunks;     // [first, last) into wg_frames
    wg::FrameRef *d_wg_frames = nullptr;
    std::vector<wg::FrameRef> wg_tasks;               // split transforms (wl.r0 > 0): (frame, sub-transform pair) records, chunk after chunk
    std::vector<std::pair<long long, long long>> wg_task_chunks;
    wg::FrameRef *d_wg_tasks = nullptr;
    long long wg_rows = 0;           // spectrum rows of the largest chunk
    long long mid_off_step = -1;
    long long n_tiles = 0, n_chunks = 0;
    std::vector<Tile> tiles_host;    // host copy of the tile list (plans built for a ranged launch only)
    XcdPlan xcd;                     // balanced plans of the fast family: placement of the short runs by XCD (lib_xcd_order.hpp)
};

static std::atomic<int> g_live_plans{0};          // plans hold raw pointers into the device's table sets (freed outside g_mu too)
static void plan_free(paa_plan *p) {
    if (!p) return;
    --g_live_plans;
    // (the caller has synchronised the stream the plan ran on: pooled blocks may be handed to the next plan at once)
    pool_free(p->d_block);          // clips, tiles, statistics chunks / partials, clip constants: one pooled block
    pool_free(p->d_mid_off);
    pool_free(p->d_wg_frames);
    pool_free(p->d_wg_tasks);
    pool_free(p->xcd.d_probe);
    xcd_plan_free(p->xcd);
    if (!p->blob_cached) pool_free(p->fam.d_blob);
    if (p->d_big) (void)hipFree(p->d_big);
    delete p;
}

// deleter of the per-call plans of the host-buffer entry points: an early error return may leave kernels of this call in
// flight on the lane's stream, and the plan's pooled blocks go straight to the next plan
static void plan_free_synced(paa_plan *p) {
    if (!p) return;
    if (cs()) (void)hipStreamSynchronize(cs());
    plan_free(p);
}

// force_params: clip_params_kernel runs whatever norms_inline says (paa_debug_plan_clip_norms reads its output)
static int launch_stats(paa_plan *p, const void *d_packed, bool force_params = false) {
    if (p->n_chunks > 0) {
        if (p->sample_kind == 0)
            hipLaunchKernelGGL(clip_stats_i16_kernel, dim3((unsigned)p->n_chunks), dim3(256), 0, cs(),
                               (const int16_t *)d_packed, p->d_chunks, (long long *)p->d_psum, (int *)p->d_pmin,
                               (int *)p->d_pmax);
        else if (p->sample_kind == 2)
            hipLaunchKernelGGL(clip_stats_stereo_kernel, dim3((unsigned)p->n_chunks), dim3(256), 0, cs(),
                               (const stereo16 *)d_packed, p->d_chunks, (long long *)p->d_psum, (int *)p->d_pmin,
                               (int *)p->d_pmax);
        else
            hipLaunchKernelGGL(clip_stats_f64_kernel, dim3((unsigned)p->n_chunks), dim3(256), 0, cs(),
                               (const double *)d_packed, p->d_chunks, (double *)p->d_psum, (double *)p->d_pmin,
                               (double *)p->d_pmax);
    }
    const unsigned gb = (unsigned)p->n_clips;
    if (p->P.norms_inline && !force_params) {
        HIP_TRY(hipGetLastError());
        return PAA_OK;
    }
    if (p->sample_kind == 1)
        hipLaunchKernelGGL((clip_params_kernel<double, double>), dim3(gb), dim3(64), 0, cs(), p->d_clips,
                           p->n_clips, (const double *)p->d_psum, (const double *)p->d_pmin,
                           (const double *)p->d_pmax, sample_scale<double>(), p->P.W, p->d_norms);
    else
        hipLaunchKernelGGL((clip_params_kernel<long long, int>), dim3(gb), dim3(64), 0, cs(), p->d_clips,
                           p->n_clips, (const long long *)p->d_psum, (const int *)p->d_pmin, (const int *)p->d_pmax,
                           p->sample_kind == 2 ? sample_scale<stereo16>() : sample_scale<int16_t>(), p->P.W, p->d_norms);
    HIP_TRY(hipGetLastError());
    return PAA_OK;
}

// the scratch of the big-window paths: p->d_big holds at least `need` bytes; *fresh: the block is a new one (its contents are
// undefined).  A plan whose allocation failed is left without a block, big_bytes = 0: its next execute allocates again
static int grow_big(paa_plan *p, size_t need, bool *fresh) {
    *fresh = false;
    if (need <= p->big_bytes) return PAA_OK;
    if (p->d_big) {
        HIP_TRY(hipStreamSynchronize(cs()));          // (kernels of the last execute may still use the old block)
        (void)hipFree(p->d_big);
        p->d_big = nullptr;
        p->big_bytes = 0;
    }
    HIP_TRY(hipMalloc(&p->d_big, need));
    p->big_bytes = need;
    *fresh = true;
    return PAA_OK;
}

// the scratch budget of the big-window paths and what follows from it (one formula each; paa_debug_big_plan reports them):
// run_big keeps per frame two packed-complex sequences (Nc double2 each), one spectrum row (Nf doubles) and three time features;
// a chunk is at most a launch's gridDim.y and never more than the longest clip
constexpr long long kBigScratchBytes = 1LL << 30;
static size_t big_frame_bytes(long long Nc, long long Nf) { return (size_t)Nc * 32 + (size_t)Nf * 8 + 24; }
static long long big_chunk_frames(long long Nc, long long Nf, long long max_frames) {
    const long long C = (long long)std::max<size_t>(1, (size_t)kBigScratchBytes / big_frame_bytes(Nc, Nf));
    return std::min<long long>(std::min<long long>(C, 65535), std::max<long long>(max_frames, 1));
}
// (one spectrum row more than frames: row 0 of a chunk is the previous chunk's last)
static size_t big_scratch_bytes(long long Nc, long long Nf, long long C) {
    return (size_t)C * Nc * 32 + (size_t)(C + 1) * Nf * 8 + (size_t)C * 24 + 256;
}
// wg_build_work (lib_dispatch.hpp): frames of a chunk of the workgroup-wide paths, one spectrum row of Nf doubles each
static long long wg_chunk_frames(long long Nf) { return std::max<long long>(2, kBigScratchBytes / (Nf * 8)); }

// windows beyond the LDS envelope: chunked Stockham passes through HBM scratch (kernels_big.hpp)
template <typename T>
static int run_big(paa_plan *p, const void *d_packed, double *d_out) {
    const PlanDev &P = p->P;
    const long long Nc = P.Nc, Nf = P.Nf;
    long long maxT = 0;
    for (auto &cd : p->clips) maxT = std::max<long long>(maxT, cd.T);
    const long long C = big_chunk_frames(Nc, Nf, maxT);
    const size_t need = big_scratch_bytes(Nc, Nf, C);
    bool fresh;
    { const int rc_g = grow_big(p, need, &fresh); if (rc_g) return rc_g; }
    double2 *bufA = reinterpret_cast<double2 *>(p->d_big);
    double2 *bufB = bufA + C * Nc;
    double *spec = reinterpret_cast<double *>(bufB + C * Nc);
    double *tfeat = spec + (C + 1) * Nf;
    const unsigned gx = (unsigned)std::min<long long>(64, (std::max<long long>(Nc, P.W) + 255) / 256);
    for (long long c = 0; c < p->n_clips; ++c) {
        const ClipDev &cd = p->clips[c];
        const T *x0 = (const T *)d_packed + cd.sample_off + P.frame_origin;
        double *oc = d_out + cd.out_off;
        long long prev_n = 0;
        for (long long t0 = 0; t0 < cd.T; t0 += C) {
            const long long n = std::min<long long>(C, cd.T - t0);
            if (t0 > 0 && P.mode != 1)       // carry the last spectrum of the previous chunk into row 0
                HIP_TRY(hipMemcpyAsync(spec, spec + prev_n * Nf, (size_t)Nf * 8, hipMemcpyDeviceToDevice, cs()));
            hipLaunchKernelGGL(big_load_kernel<T>, dim3(gx, (unsigned)n), dim3(256), 0, cs(), P, x0, t0, ClipNorm(),
                               p->d_norms, (int)c, bufA);
            if (P.mode == 0)
                hipLaunchKernelGGL(big_time_kernel, dim3((unsigned)n), dim3(64), 0, cs(), P, bufA, tfeat);
            double2 *src = bufA, *dst = bufB;
            int Ns = 1;
            for (int q = 0; q < P.n_pass; ++q) {
                hipLaunchKernelGGL(big_pass_kernel, dim3(gx, (unsigned)n), dim3(256), 0, cs(), (int)Nc, P.radix[q], Ns,
                                   P.tw, src, dst);
                Ns *= P.radix[q];
                std::swap(src, dst);
            }
            if (P.mode == 1) {
                hipLaunchKernelGGL(big_post_kernel, dim3(gx, (unsigned)n), dim3(256), 0, cs(), P, src, oc, t0);
            } else {
                hipLaunchKernelGGL(big_post_kernel, dim3(gx, (unsigned)n), dim3(256), 0, cs(), P, src, spec, 1LL);
                hipLaunchKernelGGL(big_feat_kernel, dim3((unsigned)n), dim3(64), 0, cs(), P, spec, tfeat, t0,
                                   (long long)cd.T, oc);
            }
            HIP_TRY(hipGetLastError());
            prev_n = n;
        }
        if (P.mode == 0 && P.deltas) {
            const long long items = (long long)kBase * cd.T;
            hipLaunchKernelGGL(big_delta_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, cs(),
                               (long long)cd.T, oc);
            HIP_TRY(hipGetLastError());
        }
    }
    return PAA_OK;
}

// paa_prof_enable(n): every n-th feature-kernel launch is bracketed by an event pair on the calling thread's stream (g_mu held
// by the caller); the closing event is recorded when the scope ends, i.e. right behind the launch
struct ProfScope {
    hipEvent_t stop = nullptr;
    int begin() {
        if (!(g_prof && (g_prof_seen++ % g_prof) == 0)) return PAA_OK;
        if (g_prof_used == g_prof_ev.size()) {
            hipEvent_t a, b;
            HIP_TRY(hipEventCreate(&a));
            HIP_TRY(hipEventCreate(&b));
            g_prof_ev.emplace_back(a, b);
        }
        const hipEvent_t start = g_prof_ev[g_prof_used].first;
        stop = g_prof_ev[g_prof_used].second;
        ++g_prof_used;
        HIP_TRY(hipEventRecord(start, cs()));
        return PAA_OK;
    }
    // closes the bracket here, behind the launches queued so far (else: where the scope ends)
    void end() {
        if (stop) (void)hipEventRecord(stop, cs());
        stop = nullptr;
    }
    ~ProfScope() { end(); }
};

// a launch helper of family_launch.hpp returned -1 for the plan's kernel (`of`: which of its kernels, if not the first)
static int launch_failed(const paa_plan *p, const char *of = "") {
    return fail(PAA_ERR_HIP, "launch of %s%s failed: %s", of, p->fam.kernel_name.c_str(), hipGetErrorString(hipGetLastError()));
}

// the delta rows of every clip of a features plan with deltas (kernels_wg.hpp: wg_delta_kernel), behind every workgroup-wide path
static int launch_wg_deltas(paa_plan *p, double *d_out) {
    if (p->P.mode != 0 || !p->P.deltas) return PAA_OK;
    long long maxT = 0;
    for (auto &cd : p->clips) maxT = std::max<long long>(maxT, cd.T);
    const long long gx = ((long long)kBase * maxT + 255) / 256;
    if (gx > 0x7fffffffLL)
        return fail(PAA_ERR_UNSUPPORTED, "delta grid too large (%lld frames in one clip)", maxT);
    // gridDim.y holds at most 65 535 clips: larger batches go in blocks (advisor, round 5: they used to be refused here
    // although run_big, which took them before round 5, loops the same way)
    for (long long c0 = 0; c0 < p->n_clips; c0 += 65535) {
        const unsigned ny = (unsigned)std::min<long long>(65535, p->n_clips - c0);
        hipLaunchKernelGGL(wg::wg_delta_kernel, dim3((unsigned)gx, ny), dim3(256), 0, cs(), p->d_clips + c0, d_out);
        HIP_TRY(hipGetLastError());
    }
    return PAA_OK;
}

// ---- windows beyond the one-wave kernels whose transform fits one workgroup's LDS: per chunk of frames (lib_dispatch.hpp:
// wg_build_work) one launch for the spectra of ALL its frames and one for their features, then one for the delta rows of all
// clips.  Three paths, one function each: run_wg_lds (kernels_wg.hpp, the whole transform in LDS), run_wg_split (kernels_wg.hpp,
// r0 sub-transforms) and run_wgs (kernels_wgs.hpp, the register split of r0 x q samples)
// p->d_big of the three: [spec: Nf doubles per row | tfeat: 3 per row | psum: psum_row per row | the split transforms' task
// counters: 256 bytes], a row per frame of the plan's largest chunk
struct WgBig {
    WgScratch s;
    int *counters;
    bool fresh;          // the block is a new one: nothing in it is zero
};
static int wg_scratch(paa_plan *p, size_t psum_row, WgBig &b) {
    const size_t rows = (size_t)p->wg_rows;
    const size_t o_tfeat = rows * (size_t)p->P.Nf, o_psum = o_tfeat + 3 * rows, o_counters = o_psum + psum_row * rows;      // in doubles
    const int rc = grow_big(p, o_counters * 8 + 256, &b.fresh);
    if (rc) return rc;
    double *base = reinterpret_cast<double *>(p->d_big);
    b.s = WgScratch{base, base + o_tfeat, base + o_psum};
    b.counters = reinterpret_cast<int *>(base + o_counters);
    return PAA_OK;
}
// chunk ci of the plan's frame list and -- split transforms -- of its task list, on the device
struct WgChunk {
    const wg::FrameRef *frames, *tasks;
    int n, nt;
};
static WgChunk wg_chunk(const paa_plan *p, size_t ci) {
    const auto &ch = p->wg_chunks[ci];
    const auto tc = ci < p->wg_task_chunks.size() ? p->wg_task_chunks[ci] : std::pair<long long, long long>(0, 0);
    return WgChunk{p->d_wg_frames + ch.first, p->d_wg_tasks + tc.first, (int)(ch.second - ch.first), (int)(tc.second - tc.first)};
}

// A code object holds its kernels in the order of their first use in the translation unit, and that order is part of the device code
// the GPU runs validated (scripts/device_code_hash.py, tests/test_abi_cpu.py::test_device_code_is_the_validated_one): kernels_wg.hpp's
// instances of one sample type are first named here, before the launchers below (fam_wg_execute)
template <typename T>
static void wg_kernel_order() {
    const void *const order[] = {(const void *)&wg::wg_spectrum_kernel<T, 512>, (const void *)&wg::wg_spectrum_kernel<T, 768>,
                                 (const void *)&wg::wg_split_kernel<T, 512>, (const void *)&wg::wg_split_kernel<T, 768>,
                                 (const void *)&wg::wg_feat_kernel<true>, (const void *)&wg::wg_time_kernel<T>,
                                 (const void *)&wg::wg_feat_kernel<false>};
    (void)order;
}
// kernels_wg.hpp's kernels, one launcher (and one LDS attribute) per instance
template <typename T, int NT>
static int wg_spectrum(const paa_plan *p, const WgArgs &a, const WgChunk &c, const WgScratch &s) {
    static LdsAttrCache attr;
    const wg::WgLayout &wl = p->fam.wl;
    // persistent workgroups: as many as the LDS footprint lets the chip hold at once, each walks frames b, b + grid, ...
    const unsigned per_cu = (unsigned)std::max<size_t>(1, ((size_t)160 * 1024) / (size_t)wl.lds_bytes);
    const unsigned grid = std::min<unsigned>((unsigned)c.n, (unsigned)a.num_cu * std::min<unsigned>(per_cu, NT == 768 ? 2u : 4u));
    return wg_launch(&wg::wg_spectrum_kernel<T, NT>, attr, grid, NT, (size_t)wl.lds_bytes, a.stream, a.P, wl,
                     reinterpret_cast<const unsigned short *>(p->fam.d_blob), (const T *)a.d_packed, a.clips, a.norms, c.frames, c.n, s.spec,
                     s.tfeat, a.d_out);
}
template <typename T, int NT>
static int wg_split(const paa_plan *p, const WgArgs &a, const WgChunk &c, int *counter, const WgScratch &s) {
    static LdsAttrCache attr;
    const wg::WgLayout &wl = p->fam.wl;
    // persistent workgroups over (frame, sub-transform pair) tasks, one per CU
    const unsigned grid = std::min<unsigned>((unsigned)c.nt, (unsigned)a.num_cu);
    return wg_launch(&wg::wg_split_kernel<T, NT>, attr, grid, NT, (size_t)wl.lds_bytes, a.stream, a.P, wl,
                     reinterpret_cast<const unsigned short *>(p->fam.d_blob), (const T *)a.d_packed, a.clips, a.norms, c.tasks, c.nt, counter,
                     s.spec, a.d_out);
}
template <bool STAGED>          // (wl.feat_staged)
static int wg_feat(const paa_plan *p, const WgArgs &a, const WgChunk &c, const WgScratch &s) {
    static LdsAttrCache attr;
    return wg_launch(&wg::wg_feat_kernel<STAGED>, attr, (unsigned)c.n, wg::kFeatThreads, (size_t)p->fam.wl.feat_lds_bytes, a.stream, a.P,
                     c.frames, a.clips, s.spec, s.tfeat, a.d_out);
}

// (in all three, bench.py's event pairs bracket the spectrum kernel: the dominant one of the path)
template <typename T>
static int run_wg_lds(paa_plan *p, const WgArgs &a) {
    WgBig b;
    { const int rc_b = wg_scratch(p, 0, b); if (rc_b) return rc_b; }
    for (size_t ci = 0; ci < p->wg_chunks.size(); ++ci) {
        const WgChunk c = wg_chunk(p, ci);
        ProfScope prof_scope;
        { const int rc_p = prof_scope.begin(); if (rc_p) return rc_p; }
        if (p->fam.wl.threads == 768 ? wg_spectrum<T, 768>(p, a, c, b.s) : wg_spectrum<T, 512>(p, a, c, b.s)) return launch_failed(p);
        prof_scope.end();
        if (a.P.mode != 1 && (p->fam.wl.feat_staged ? wg_feat<true>(p, a, c, b.s) : wg_feat<false>(p, a, c, b.s)))
            return launch_failed(p, "the feature kernel of ");
    }
    return launch_wg_deltas(p, a.d_out);
}

template <typename T>
static int run_wg_split(paa_plan *p, const WgArgs &a) {
    WgBig b;
    { const int rc_b = wg_scratch(p, 0, b); if (rc_b) return rc_b; }
    for (size_t ci = 0; ci < p->wg_chunks.size(); ++ci) {
        const WgChunk c = wg_chunk(p, ci);
        ProfScope prof_scope;
        { const int rc_p = prof_scope.begin(); if (rc_p) return rc_p; }
        HIP_TRY(hipMemsetAsync(b.counters, 0, sizeof(int), a.stream));
        if (p->fam.wl.threads == 768 ? wg_split<T, 768>(p, a, c, b.counters, b.s) : wg_split<T, 512>(p, a, c, b.counters, b.s))
            return launch_failed(p);
        prof_scope.end();
        if (a.P.mode == 0) {
            hipLaunchKernelGGL((wg::wg_time_kernel<T>), dim3((unsigned)c.n), dim3(64 * wg::kTimeWaves), 0, a.stream, a.P, (const T *)a.d_packed,
                               a.clips, a.norms, c.frames, b.s.tfeat);
            HIP_TRY(hipGetLastError());
        }
        if (a.P.mode != 1 && (p->fam.wl.feat_staged ? wg_feat<true>(p, a, c, b.s) : wg_feat<false>(p, a, c, b.s)))
            return launch_failed(p, "the feature kernel of ");
    }
    return launch_wg_deltas(p, a.d_out);
}

static int run_wgs(paa_plan *p, const WgArgs &a, const wgs::Sel &ws) {
    WgBig b;
    { const int rc_b = wg_scratch(p, (size_t)(ws.r0 / 2) * 4, b); if (rc_b) return rc_b; }
    // (kernels_wgs.hpp: one counter per XCD segment + the workgroups that are done; its last workgroup leaves them at zero)
    if (b.fresh) HIP_TRY(hipMemsetAsync(b.counters, 0, 16 * sizeof(int), a.stream));
    for (size_t ci = 0; ci < p->wg_chunks.size(); ++ci) {
        const WgChunk c = wg_chunk(p, ci);
        ProfScope prof_scope;
        { const int rc_p = prof_scope.begin(); if (rc_p) return rc_p; }
        if (launch::wgs(ws.r0, ws.q, c.tasks, c.nt, b.counters, b.s, a)) return launch_failed(p);
        prof_scope.end();
        // (the time-domain features are formed in the kernel's {1, 2} tasks)
        if (a.P.mode != 1 && launch::wgs_feat(ws.r0, ws.q, c.frames, c.n, b.s, a)) return launch_failed(p, "the feature kernel of ");
    }
    return launch_wg_deltas(p, a.d_out);
}

// the fused three-pass kernel (kernels_wgr.hpp): ONE launch for all frames of all clips, then the delta rows
static int run_wgr(paa_plan *p, const WgArgs &a, const Tile *runs, long long n_runs) {
    if (n_runs > 0) {
        ProfScope prof_scope;
        { const int rc_p = prof_scope.begin(); if (rc_p) return rc_p; }
        if (launch::wgr(wgr::wgr_shape_id(a.P.W), a.P.mode, runs, n_runs, reinterpret_cast<const wgr::WgrTab *>(p->fam.d_blob), a))
            return launch_failed(p);
    }
    return launch_wg_deltas(p, a.d_out);
}

#include "lib_dispatch.hpp"

// ranges > 1: the caller will launch the plan's tiles in that many consecutive groups (run_host_st's copy-back pipeline)
static int plan_build(const int64_t *offsets, int64_t n_clips, int sample_kind, double fs, int window, int step,
                      int deltas, int mode, paa_plan **out, int ranges = 1, bool resident = false) {
    int rc = ensure_init();
    if (rc) return rc;
    if (!offsets || n_clips < 1 || !out) return fail(PAA_ERR_ARG, "null offsets / no clips");
    if (window < 2 || step < 1) return fail(PAA_ERR_ARG, "window=%d step=%d: need window >= 2, step >= 1", window, step);
    if (sample_kind < 0 || sample_kind > 2)
        return fail(PAA_ERR_ARG, "sample_kind must be 0 (int16), 1 (float64) or 2 (interleaved stereo int16)");
    if (!(fs > 0)) return fail(PAA_ERR_ARG, "sampling rate must be positive");
    std::unique_ptr<paa_plan, void (*)(paa_plan *)> p(new paa_plan(), plan_free);
    ++g_live_plans;
    p->n_clips = n_clips;
    p->sample_kind = sample_kind;
    p->mode = mode;
    p->xcd.resident = resident;
    TableSet *tab = nullptr;
    if ((rc = get_tables(fs, window, mode == 0, mode != 1, &tab))) return rc;
    p->tab = tab;
    const int Nf = window / 2;
    const int F = (mode == 0) ? kBase * (deltas ? 2 : 1) : 0;
    p->row_width = (mode == 1) ? Nf : (mode == 2 ? 12 : 0);

    // ---- clips
    p->clips.resize(n_clips);
    p->alloc_rows.assign(n_clips, 0);
    long long out_off = 0, total_frames = 0, n_chunks = 0;
    p->stat_chunk = stat_chunk_for(offsets[n_clips] - offsets[0], g_num_cu);
    const int kChunk = p->stat_chunk;
    for (int64_t c = 0; c < n_clips; ++c) {
        const long long n = offsets[c + 1] - offsets[c];
        if (n < 0) return fail(PAA_ERR_ARG, "offsets must be non-decreasing (clip %lld)", (long long)c);
        ClipDev &cd = p->clips[c];
        cd.sample_off = offsets[c];
        cd.n = n;
        cd.out_off = out_off;
        long long T = 0, rows = 0;
        if (mode == 0) {
            T = paa_num_frames(n, window, step);
            if (T < 1)
                return fail(PAA_ERR_TOO_SHORT, "need at least one array to concatenate (clip %lld has %lld samples, "
                            "window %d)", (long long)c, n, window);
            rows = T;
            out_off += (long long)F * T;
        } else {
            int64_t filled = 0;
            rows = (mode == 1) ? paa_spectrogram_rows(n, window, step, &filled)
                               : paa_chromagram_rows(n, window, step, &filled);
            if (rows < 1)
                return fail(PAA_ERR_TOO_SHORT, "signal too short for window %d / step %d (clip %lld, %lld samples)",
                            window, step, (long long)c, n);
            // full-length frames only; a truncated chromagram tail frame is added by the caller
            long long full = 0;
            for (long long pos = window; pos + window <= n && full < filled; pos += step) ++full;
            T = full;
            out_off += rows * p->row_width;
        }
        if (T > 0x7fffffffLL) return fail(PAA_ERR_ARG, "clip %lld has too many frames", (long long)c);
        p->alloc_rows[c] = rows;
        cd.T = (int)T;
        cd.stat_first = (int)n_chunks;
        cd.stat_count = (int)((n + kChunk - 1) / kChunk);
        cd.pad = 0;
        n_chunks += cd.stat_count;
        total_frames += T;
    }
    p->total_frames = total_frames;
    p->out_doubles = out_off;
    p->n_chunks = n_chunks;

    // ---- device plan
    PlanDev &P = p->P;
    memset(&P, 0, sizeof(P));
    P.W = window; P.S = step; P.Nf = Nf; P.Nc = tab->fft.len; P.even = tab->fft.even;
    P.n_pass = (int)tab->fft.radix.size();
    if (P.n_pass > 24) return fail(PAA_ERR_UNSUPPORTED, "window %d needs more than 24 FFT passes", window);
    for (int i = 0; i < P.n_pass; ++i) P.radix[i] = tab->fft.radix[i];
    P.tw = tab->d_tw; P.post = tab->d_post;
    P.mel_lo = tab->d_mel_lo; P.mel_cnt = tab->d_mel_cnt; P.mel_off = tab->d_mel_off; P.mel_w = tab->d_mel_w;
    P.dct = tab->d_dct; P.ch_start = tab->d_ch_start; P.ch_src = tab->d_ch_src; P.ch_w = tab->d_ch_w;
    P.fs = fs; P.deltas = deltas ? 1 : 0; P.F = F;
    P.blk_t = window / 10; P.blk_f = Nf / 10;
    P.mode = mode;
    P.frame_origin = (mode == 0) ? 0 : window;
    { const char *dbg = experiment_env("PAA_KERNEL_DEBUG"); P.debug = dbg ? atoi(dbg) : 0; }

    // ---- kernel choice (the first entry of kFamilies that takes the shape) and its work list
    FamilyCtx fc{p.get(), tab, fs, window, step, deltas, mode, sample_kind, F, total_frames, ranges};
    if ((rc = choose_family(fc))) return rc;
    const Family &fam = kFamilies[p->fam.family];
    std::vector<Tile> tiles;
    if ((rc = fam.work(fc, tiles))) return rc;
    p->n_tiles = (long long)tiles.size();
    if (ranges > 1 && fam.ranged) p->tiles_host = tiles;          // (the host pipeline cuts the list at frame boundaries)
    if (p->n_tiles > 0x7fffffffLL || n_chunks > 0x7fffffffLL || n_clips > 0x7fffffffLL)
        return fail(PAA_ERR_UNSUPPORTED, "batch too large for one launch (%lld runs, %lld statistics chunks, %lld clips)",
                    p->n_tiles, n_chunks, (long long)n_clips);
    std::vector<StatChunk> chunks;
    chunks.reserve((size_t)n_chunks);
    for (int64_t c = 0; c < n_clips; ++c)
        for (int i = 0; i < p->clips[c].stat_count; ++i) {
            StatChunk ch; ch.start = p->clips[c].sample_off + (long long)i * kChunk;
            ch.len = (int)std::min<long long>(kChunk, p->clips[c].n - (long long)i * kChunk);
            ch.clip = (int)c;
            chunks.push_back(ch);
        }
    // ONE pooled device block and ONE upload per plan (the host-buffer entry points build a plan per call):
    //   [clip descriptors | tiles | statistics chunks] (uploaded) [clip constants | partial sums | minima | maxima]
    {
        const size_t nch = (size_t)std::max<long long>(n_chunks, 1);
        const size_t o_clips = 0, o_tiles = o_clips + up256(p->clips.size() * sizeof(ClipDev));
        const size_t o_chunks = o_tiles + up256(std::max<size_t>(tiles.size(), 1) * sizeof(Tile));
        const size_t o_norms = o_chunks + up256(std::max<size_t>(chunks.size(), 1) * sizeof(StatChunk));
        const size_t o_sum = o_norms + up256((size_t)n_clips * sizeof(ClipNorm));
        const size_t o_min = o_sum + up256(nch * 8), o_max = o_min + up256(nch * 8), total = o_max + up256(nch * 8);
        if ((rc = pool_alloc(&p->d_block, total))) return rc;
        std::vector<unsigned char> stage(o_norms, 0);
        memcpy(stage.data() + o_clips, p->clips.data(), p->clips.size() * sizeof(ClipDev));
        if (!tiles.empty()) memcpy(stage.data() + o_tiles, tiles.data(), tiles.size() * sizeof(Tile));
        if (!chunks.empty()) memcpy(stage.data() + o_chunks, chunks.data(), chunks.size() * sizeof(StatChunk));
        HIP_TRY(hipMemcpy(p->d_block, stage.data(), o_norms, hipMemcpyHostToDevice));
        unsigned char *b = reinterpret_cast<unsigned char *>(p->d_block);
        p->d_clips = reinterpret_cast<ClipDev *>(b + o_clips);
        p->d_tiles = reinterpret_cast<Tile *>(b + o_tiles);
        p->d_chunks = reinterpret_cast<StatChunk *>(b + o_chunks);
        p->d_norms = reinterpret_cast<ClipNorm *>(b + o_norms);
        p->d_psum = b + o_sum; p->d_pmin = b + o_min; p->d_pmax = b + o_max;
    }
    // the one-wave feature kernels fold the statistics partials into the clip constants themselves (their waves' prologue);
    // chromagram plans keep clip_params_kernel (the truncated-tail kernel of the host entry point reads its output), and so
    // do the big-window paths
    P.st_sum = p->d_psum; P.st_min = p->d_pmin; P.st_max = p->d_pmax;
    P.st_scale = sample_kind == 1 ? sample_scale<double>() : (sample_kind == 2 ? sample_scale<stereo16>() : sample_scale<int16_t>());
    P.norms_inline = (fam.norms_inline && mode != 2) ? 1 : 0;
    *out = p.release();
    return PAA_OK;
}

extern "C" int paa_plan_execute(paa_plan_t *plan, const void *d_packed, double *d_out) {
    if (!plan || !d_packed || !d_out) return fail(PAA_ERR_ARG, "null plan / buffer");
    { const int rc_init = ensure_init(); if (rc_init) return rc_init; }
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = comm_wait_buffer_free(d_out);      // a gather of this buffer may still be in flight
    if (rc) return rc;
    rc = launch_stats(plan, d_packed);
    if (rc) return rc;
    return kFamilies[plan->fam.family].execute(plan, d_packed, d_out, plan->d_tiles, plan->n_tiles);
}

extern "C" int paa_plan_create(const int64_t *offsets, int64_t n_clips, int sample_kind, double fs, int window,
                               int step, int deltas, paa_plan_t **out_plan) {
    std::lock_guard<std::mutex> lk(g_mu);
    return plan_build(offsets, n_clips, sample_kind, fs, window, step, deltas, 0, out_plan, 1, true);
}

// device-resident plan of the spectrogram (mode 1, :389-452) / chromagram (mode 2, :324-386) rows of one or more clips:
// full-length frames only, row t of a clip at out + out_offset(clip) + t * row_width (Nf or 12 doubles); rows the reference
// allocates but never fills, and the truncated chromagram tail frame, are the host entry points' business
extern "C" int paa_plan_create_mode(const int64_t *offsets, int64_t n_clips, int sample_kind, double fs, int window,
                                    int step, int mode, paa_plan_t **out_plan) {
    if (mode < 0 || mode > 2) return fail(PAA_ERR_ARG, "mode must be 0 (features), 1 (spectrogram) or 2 (chromagram)");
    std::lock_guard<std::mutex> lk(g_mu);
    return plan_build(offsets, n_clips, sample_kind, fs, window, step, 0, mode, out_plan);
}

extern "C" int paa_plan_destroy(paa_plan_t *plan) {
    if (g_device.load() >= 0) (void)ensure_init();       // (binds the calling thread to the library's device)
    std::lock_guard<std::mutex> lk(g_mu);
    if (cs()) (void)hipStreamSynchronize(cs());
    plan_free(plan);
    return PAA_OK;
}

extern "C" int64_t paa_plan_total_frames(const paa_plan_t *plan) { return plan ? plan->total_frames : 0; }
extern "C" int64_t paa_plan_out_doubles(const paa_plan_t *plan) { return plan ? plan->out_doubles : 0; }
extern "C" const char *paa_plan_kernel_name(const paa_plan_t *plan) { return plan ? plan->fam.kernel_name.c_str() : ""; }

extern "C" int paa_plan_out_offsets(const paa_plan_t *plan, int64_t *out_offsets) {
    if (!plan || !out_offsets) return fail(PAA_ERR_ARG, "null plan / buffer");
    for (long long c = 0; c < plan->n_clips; ++c) out_offsets[c] = plan->clips[c].out_off;
    return PAA_OK;
}

extern "C" int64_t paa_plan_mid_doubles(const paa_plan_t *plan, int64_t mid_step_ratio) {
    if (!plan || mid_step_ratio < 1) return 0;
    long long tot = 0;
    for (long long c = 0; c < plan->n_clips; ++c)
        tot += 2LL * plan->P.F * paa_num_mid_windows(plan->clips[c].T, mid_step_ratio);
    return tot;
}

extern "C" int paa_plan_mid_execute(paa_plan_t *plan, const double *d_st, int64_t mid_ratio, int64_t mid_step_ratio,
                                    double *d_mid) {
    if (!plan || !d_st || !d_mid) return fail(PAA_ERR_ARG, "null plan / buffer");
    { const int rc_init = ensure_init(); if (rc_init) return rc_init; }
    if (plan->mode != 0) return fail(PAA_ERR_ARG, "mid-term statistics need a feature plan");
    if (mid_step_ratio < 1)
        return fail(PAA_ERR_ARG, "mid_step / short_step rounds to %lld: the reference loops forever "
                    "(MidTermFeatures.py:102,124)", (long long)mid_step_ratio);
    std::lock_guard<std::mutex> lk(g_mu);
    { const int rc_w = comm_wait_buffer_free(d_mid); if (rc_w) return rc_w; }      // a gather of this buffer may still read it
    long long maxM = 0;
    if (plan->mid_off_step != mid_step_ratio) {
        std::vector<long long> off(plan->n_clips);
        long long o = 0;
        for (long long c = 0; c < plan->n_clips; ++c) {
            off[c] = o;
            o += 2LL * plan->P.F * paa_num_mid_windows(plan->clips[c].T, mid_step_ratio);
        }
        if (cs()) HIP_TRY(hipStreamSynchronize(cs()));
        int rc = upload_pooled(&plan->d_mid_off, off.data(), off.size());
        if (rc) return rc;
        plan->mid_off_step = mid_step_ratio;
    }
    for (long long c = 0; c < plan->n_clips; ++c)
        maxM = std::max<long long>(maxM, paa_num_mid_windows(plan->clips[c].T, mid_step_ratio));
    const long long items = (long long)plan->P.F * maxM;
    const int bpc = (int)((items + 15) / 16);          // 16 (row, window) items per 256-thread block
    const long long grid = plan->n_clips * bpc;
    if (grid > 0x7fffffffLL) return fail(PAA_ERR_UNSUPPORTED, "mid-term grid too large");
    hipLaunchKernelGGL(mid_stats_kernel, dim3((unsigned)grid), dim3(256), 0, cs(), plan->d_clips, plan->d_mid_off,
                       d_st, plan->P.F, (long long)mid_ratio, (long long)mid_step_ratio, bpc, d_mid);
    HIP_TRY(hipGetLastError());
    return PAA_OK;
}

// beat rate of every clip of an executed plan (deltas on or off: rows 0..18 are used)
extern "C" int paa_plan_beat_execute(paa_plan_t *plan, const double *d_st, double window_size, double *d_beat) {
    if (!plan || !d_st || !d_beat) return fail(PAA_ERR_ARG, "null plan / buffer");
    if (plan->mode != 0) return fail(PAA_ERR_ARG, "beat extraction needs a feature plan");
    if (!(window_size > 0)) return fail(PAA_ERR_ARG, "window_size must be positive");
    { const int rc_init = ensure_init(); if (rc_init) return rc_init; }
    const int max_beat = (int)nearbyint(2.0 / window_size);          // int(round(2.0 / window_size)), :33
    // no bins (window_size >= 4 s): the reference's np.argmax of the empty histogram raises ValueError (:68)
    if (max_beat < 1) return fail(PAA_ERR_ARG, "attempt to get argmax of an empty sequence (beat histogram of %d bins)", max_beat);
    if (max_beat > 4096) return fail(PAA_ERR_UNSUPPORTED, "beat histogram of %d bins", max_beat);
    std::lock_guard<std::mutex> lk(g_mu);
    { const int rc_w = comm_wait_buffer_free(d_beat); if (rc_w) return rc_w; }
    const size_t lds = (size_t)kBeatRows * (kBeatTile + 1) * 8 + (size_t)kBeatRows * max_beat * 4;
    if (lds > 160 * 1024)
        return fail(PAA_ERR_UNSUPPORTED, "beat histogram of %d bins needs %zu bytes of LDS (160 KB per workgroup)", max_beat, lds);
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&beat_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(beat_kernel, dim3((unsigned)plan->n_clips), dim3(64), lds, cs(), plan->d_clips, d_st,
                       window_size, max_beat, d_beat);
    HIP_TRY(hipGetLastError());
    return PAA_OK;
}

// [34][T_c] base slabs of n_clips clips, back to back -> [68][T_c] slabs back to back (delta rows re-formed on the device;
// bit-identical to what a 68-row plan stores).  Queued behind everything on the communication stream when a communicator
// exists (the slabs usually arrive through paa_comm_gatherv_f64), else on the library stream.  The tile list of the last
// frames[] is kept (a sharded job expands the same batch shape step after step).
struct DeltaPlanCache {
    std::vector<int64_t> frames;
    DeltaTile *d_tiles = nullptr;
    long long n_tiles = 0;
};
static DeltaPlanCache g_delta_cache;
static hipStream_t comm_stream_or_null();
static int comm_order_after_compute(hipStream_t s);
extern "C" int paa_dev_expand_deltas(const double *d_base, const int64_t *frames, int64_t n_clips, double *d_out) {
    if (!d_base || !frames || !d_out || n_clips < 1) return fail(PAA_ERR_ARG, "null buffer / no clips");
    if (d_base == d_out) return fail(PAA_ERR_ARG, "in-place expansion is not possible (rows move)");
    { const int rc_init = ensure_init(); if (rc_init) return rc_init; }
    std::lock_guard<std::mutex> lk(g_mu);
    DeltaPlanCache &dc = g_delta_cache;
    if ((int64_t)dc.frames.size() != n_clips || memcmp(dc.frames.data(), frames, (size_t)n_clips * 8) != 0) {
        constexpr int kTile = 2048;
        std::vector<DeltaTile> tiles;
        long long tot = 0;
        for (int64_t c = 0; c < n_clips; ++c) {
            const long long T = frames[c];
            if (T < 0 || T > 0x7fffffffLL) return fail(PAA_ERR_ARG, "clip %lld: %lld frames", (long long)c, T);
            for (long long t0 = 0; t0 < T; t0 += kTile) {
                DeltaTile tl;
                tl.base_off = (long long)kBase * tot; tl.out_off = 2LL * kBase * tot;
                tl.T = (int)T; tl.t0 = (int)t0; tl.cnt = (int)std::min<long long>(kTile, T - t0); tl.pad = 0;
                tiles.push_back(tl);
            }
            tot += T;
        }
        if (tiles.size() > 0x7fffffffULL) return fail(PAA_ERR_UNSUPPORTED, "too many tiles");
        // a launch that still reads the old list may be in flight on ANY lane's stream or on the communication stream (another
        // host thread may have queued it): the list is replaced once per batch shape, so a device-wide wait is affordable
        HIP_TRY(hipDeviceSynchronize());
        const int rc = upload_pooled(&dc.d_tiles, tiles.data(), tiles.size());
        if (rc) return rc;
        dc.n_tiles = (long long)tiles.size();
        dc.frames.assign(frames, frames + n_clips);
    }
    if (dc.n_tiles == 0) return PAA_OK;
    hipStream_t s = comm_stream_or_null();
    if (s) { const int rc_o = comm_order_after_compute(s); if (rc_o) return rc_o; }
    else s = cs();
    hipLaunchKernelGGL(expand_deltas_kernel, dim3((unsigned)dc.n_tiles, (unsigned)kBase), dim3(256), 0, s, dc.d_tiles, d_base, d_out);
    HIP_TRY(hipGetLastError());
    return PAA_OK;
}
