// Kernel choice of a plan: one table entry per feature-kernel path, walked in order by choose_family; the first entry whose
// select() takes the (window, step, sample type, mode, rows) owns the plan.  plan_build, paa_plan_execute and run_host_st only
// call through the entry.  Adding a path = one more entry.  Included by lib_plan.hpp after the plan structure and its launchers.
#pragma once

struct FamilyCtx {
    paa_plan *p;
    TableSet *tab;
    double fs;
    int window, step, deltas, mode, sample_kind, F;
    long long total_frames;
    int ranges;          // >= 1: the plan will be launched in this many consecutive tile ranges (host pipeline): runs are cut as if
                         // the chip had `ranges` times its CUs, so that every range still fills it in one round
    int num_cu() const { return g_num_cu * (ranges > 1 ? ranges : 1); }
    const MelTable *mel() const { return mode == 0 ? &tab->mel : nullptr; }
    const ChromaTable *chroma() const { return mode != 1 ? &tab->chroma : nullptr; }
};
// how the tile list cuts a clip: runs of `run` frames in multiples of `quantum`; a run with t0 > 0 is halo_inside frames
// shorter (kernels whose look-back frames ride inside the run's first iteration)
struct RunRule {
    int run = 64, quantum = 4, halo_inside = 0;
    int fill_wg_runs = 0;        // > 0: runs per workgroup of a kernel with ONE workgroup per CU -- a plan whose equal runs fill less than
                                 // one round of the chip is re-cut into num_cu x fill_wg_runs runs of two lengths (lib_plan.hpp: balanced_runs)
    int fill_min_run = 16;       // ... none of them shorter than this
    bool fill_by_xcd = false;    // ... and the short ones go to the slow XCDs (lib_xcd_order.hpp).  The fast family only: st_ct shares
                                 // fill_wg_runs but has had no A/B of the placement, it keeps the even spread
};
struct Family {
    const char *id;
    // 1: takes the shape (layout, lds and kernel_name set in `f`, the device tables -- if any -- in `blob`), 0: declines, < 0: error
    // code.  Depends only on the table set, the mode and the rows (and the fast family's step): choose_family caches the result
    int (*select)(const FamilyCtx &c, FamilyChoice &f, std::vector<unsigned char> &blob);
    // per plan, after the choice: the work list -- the tile list (one-wave families; wgr's runs) or the path's own lists on the plan
    int (*work)(FamilyCtx &c, std::vector<Tile> &tiles);
    // queues the plan's kernels on cs(); tiles / n_tiles: the plan's tile list, or a range of it
    int (*execute)(paa_plan *p, const void *d_packed, double *d_out, const Tile *tiles, long long n_tiles);
    bool ranged;          // the tile list may be launched in consecutive ranges (run_host_st's copy-back pipeline)
    bool norms_inline;    // the kernel folds the statistics partials into the clip constants (else clip_params_kernel runs first)
};

static std::string mode_kernel_name(int mode, const std::string &suffix) {
    return std::string(mode == 0 ? "st_" : (mode == 1 ? "spectrogram_" : "chromagram_")) + suffix;
}
// the usual rule of the one-frame-per-iteration kernels: about two chip-wide rounds, 8 .. 64 frames per run
static int two_round_run(long long total_frames, int waves, int num_cu) {
    const long long slots = (long long)num_cu * waves * 2;
    const long long per = (total_frames + slots - 1) / slots;
    return (int)std::min<long long>(64, std::max<long long>(8, (per + 3) / 4 * 4));
}

// the tiles of balanced_runs' lengths, clip after clip in frame order
static void balanced_tiles(const std::vector<std::vector<int>> &run_lens, std::vector<Tile> &tiles) {
    for (size_t ci = 0; ci < run_lens.size(); ++ci) {
        long long t0 = 0;
        for (int cnt : run_lens[ci]) {
            Tile tl; tl.clip = (int)ci; tl.t0 = (int)t0; tl.cnt = cnt; tl.pad = 0;
            tiles.push_back(tl);
            t0 += cnt;
        }
    }
}
// the tile list of a one-wave family: runs of its RunRule, balanced or equal, clip after clip in frame order
static void build_tiles(FamilyCtx &c, const RunRule &rr, std::vector<Tile> &tiles) {
    const std::vector<ClipDev> &clips = c.p->clips;
    const int run = rr.run, run_quantum = rr.quantum, run_halo = rr.halo_inside;
    tiles.reserve((size_t)(c.total_frames / run + clips.size()));
    std::vector<std::vector<int>> run_lens;
#ifndef PAA_BALANCED_RUNS
#define PAA_BALANCED_RUNS 1           // (0: A/B build of scripts/rounds/r05/gpu_r05w.sh -- equal runs, 250 workgroups for the one-hour clip)
#endif
    int order[kXcdLabels];
    unsigned long long epoch = 0;
    const bool by_xcd = rr.fill_by_xcd && xcd_current(order, &epoch);
    const bool balanced = PAA_BALANCED_RUNS && rr.fill_wg_runs > 0 && c.ranges <= 1 &&
                          balanced_runs(clips, run, run_quantum, run_halo, rr.fill_wg_runs, g_num_cu, rr.fill_min_run, run_lens,
                                        by_xcd ? order : nullptr);
    if (balanced) {
        balanced_tiles(run_lens, tiles);
        if (rr.fill_by_xcd) {          // what a later re-cut under another order needs (fam_fast_execute)
            XcdPlan &x = c.p->xcd;
            x.balanced = true;
            x.run = run; x.quantum = run_quantum; x.shrink = run_halo; x.wg_runs = rr.fill_wg_runs; x.min_run = rr.fill_min_run;
            x.epoch = epoch;
            xcd_label_totals(tiles.data(), (long long)tiles.size(), x.wg_runs, x.quantum, x.shrink, x.n_label);
            if (x.resident) x.tiles = tiles;
        }
        return;
    }
    for (size_t ci = 0; ci < clips.size(); ++ci) {
        const long long T = clips[ci].T;
        if (T <= 0) continue;
        const int len = clip_run_length(T, run, run_quantum);          // equal runs per clip
        for (long long t0 = 0; t0 < T;) {
            const long long want = (t0 > 0) ? len - run_halo : len;
            Tile tl; tl.clip = (int)ci; tl.t0 = (int)t0; tl.cnt = (int)std::min<long long>(want, T - t0); tl.pad = 0;
            tiles.push_back(tl);
            t0 += tl.cnt;
        }
    }
}
template <void (*Rule)(FamilyCtx &, RunRule &)>
static int tile_work(FamilyCtx &c, std::vector<Tile> &tiles) {
    RunRule rr;
    Rule(c, rr);
    build_tiles(c, rr, tiles);
    return PAA_OK;
}
// one launch of a one-wave family over a range of tiles
typedef int (*TileLaunch)(const paa_plan *p, const TileArgs &a);
template <TileLaunch Launch>
static int tile_execute(paa_plan *p, const void *d_packed, double *d_out, const Tile *tiles, long long n_tiles) {
    if (n_tiles == 0) return PAA_OK;
    ProfScope prof_scope;
    { const int rc_p = prof_scope.begin(); if (rc_p) return rc_p; }
    const TileArgs a{p->P, p->fam.d_blob, d_packed, p->sample_kind, p->d_clips, p->d_norms, tiles, n_tiles, d_out, cs()};
    return Launch(p, a) ? launch_failed(p) : PAA_OK;
}

// ---- kernels_fast.hpp: int16, window 800, step 400 / 800, features only
static int fam_fast_select(const FamilyCtx &c, FamilyChoice &f, std::vector<unsigned char> &) {
    if (c.mode != 0 || g_force_generic) return 0;
    const int rc = fast_select(c.window, c.step, c.sample_kind, c.fs, c.tab->fast, c.tab->fft, c.tab->mel, c.tab->chroma, f.fl,
                               g_f800_waves);
    if (rc < 0) return fail(rc, "building the tables of the specialised kernel failed");
    if (rc) { f.lds = f.fl.lds; f.kernel_name = f.fl.name; }
    return rc;
}
static void fam_fast_rule(FamilyCtx &c, RunRule &r) {
    // one wave per run of whole 4-frame quads, at most fl.run frames; a run after a clip's first starts its first quad one frame
    // early (two with deltas: the flux of the last halo frame feeds a delta) -- the halo rides inside the first iteration, the run
    // stores that many frames less (kernels_fast.hpp: HALO); see choose_run_cap
    const FastLaunch &fl = c.p->fam.fl;
    r.quantum = 4;
    r.halo_inside = c.deltas ? 2 : 1;
    r.run = choose_run_cap(c.p->clips, 4, 16, fl.run, 0, fl.waves_per_cu, c.num_cu(), r.halo_inside);
    r.fill_wg_runs = fl.waves_per_cu;
    r.fill_by_xcd = true;
    if (const char *rc_env = experiment_env("PAA_RUN_CAP")) r.run = std::max(16, atoi(rc_env) / 4 * 4);      // A/B experiments only
}
static int fam_fast_launch(const paa_plan *p, const TileArgs &a) {
    TileArgs af = a;          // (its tables belong to the table set, not to the choice)
    af.blob = reinterpret_cast<const unsigned char *>(p->tab->fast.d_blob);
    return launch::fast(p->fam.fl, af);
}
// ---- ... and the placement of its short runs by XCD (lib_xcd_order.hpp), for the balanced plans of paa_plan_create
// the record of the plan's last probe launch, if its copy has arrived: into the device's averages
static void xcd_consume(paa_plan *p) {
    XcdPlan &x = p->xcd;
    if (!x.probe_pending) return;
    if (hipEventQuery(x.probe_ev) != hipSuccess) { (void)hipGetLastError(); return; }      // (not ready is not an error of this execute)
    x.probe_pending = false;
    xcd_fold(x.h_probe, p->n_tiles, x.wg_runs, g_num_cu, x.pending_n);
}
// the plan's list was cut under another order than the one in force: cut it again on the host and upload it, stream-ordered in front
// of the launch that follows (the executes of a plan share a stream).  A handful of times per process
static int xcd_recut(paa_plan *p, const int *order8, unsigned long long epoch) {
    XcdPlan &x = p->xcd;
    std::vector<std::vector<int>> run_lens;
    std::vector<Tile> tiles;
    if (balanced_runs(p->clips, x.run, x.quantum, x.shrink, x.wg_runs, g_num_cu, x.min_run, run_lens, order8)) balanced_tiles(run_lens, tiles);
    x.epoch = epoch;
    if ((long long)tiles.size() != p->n_tiles) return PAA_OK;          // (cannot happen: an order moves runs, it does not add any)
    const size_t bytes = tiles.size() * sizeof(Tile);
    if (!x.h_tiles) HIP_TRY(hipHostMalloc((void **)&x.h_tiles, bytes, hipHostMallocDefault));
    if (!x.upload_ev) HIP_TRY(hipEventCreateWithFlags(&x.upload_ev, hipEventDisableTiming));
    if (x.upload_pending) HIP_TRY(hipEventSynchronize(x.upload_ev));          // (the staging buffer of the last re-cut)
    memcpy(x.h_tiles, tiles.data(), bytes);
    HIP_TRY(hipMemcpyAsync(p->d_tiles, x.h_tiles, bytes, hipMemcpyHostToDevice, cs()));
    HIP_TRY(hipEventRecord(x.upload_ev, cs()));
    x.upload_pending = true;
    xcd_label_totals(tiles.data(), p->n_tiles, x.wg_runs, x.quantum, x.shrink, x.n_label);
    x.tiles.swap(tiles);
    return PAA_OK;
}
// the probe buffers of a plan, at its first probe launch
static int xcd_probe_buffers(paa_plan *p) {
    XcdPlan &x = p->xcd;
    const size_t bytes = (size_t)p->n_tiles * 16;
    if (!x.d_probe) { const int rc = pool_alloc((void **)&x.d_probe, bytes); if (rc) return rc; }
    if (!x.h_probe) HIP_TRY(hipHostMalloc((void **)&x.h_probe, bytes, hipHostMallocDefault));
    if (!x.probe_ev) HIP_TRY(hipEventCreateWithFlags(&x.probe_ev, hipEventDisableTiming));
    return PAA_OK;
}
// force_probe: paa_debug_plan_probe's launch (the caller waits for the record itself)
static int fam_fast_execute_probe(paa_plan *p, const void *d_packed, double *d_out, const Tile *tiles, long long n_tiles, bool force_probe) {
    if (n_tiles == 0) return PAA_OK;
    XcdPlan &x = p->xcd;
    bool probe = false;
    if (x.balanced && x.resident && tiles == p->d_tiles && n_tiles == p->n_tiles) {
        if (xcd_enabled()) {
            xcd_consume(p);
            int order[kXcdLabels];
            unsigned long long epoch = 0;
            const bool on = xcd_current(order, &epoch);
            if (epoch != x.epoch) { const int rc = xcd_recut(p, on ? order : nullptr, epoch); if (rc) return rc; }
            // (the kernel's run-time-list instances carry no probe: launch::fast; a forced probe is not one of the device's own)
            probe = xcd_want_probe(p->fam.fl.layout.fixed_lists && !x.probe_pending && !force_probe);
        } else if (x.epoch != 0) {          // switched off after an ordered cut: back to the even spread
            const int rc = xcd_recut(p, nullptr, 0);
            if (rc) return rc;
        }
        probe = (probe || force_probe) && p->fam.fl.layout.fixed_lists && !x.probe_pending;
        if (probe) {
            const int rc = xcd_probe_buffers(p);
            if (rc) return rc;
            HIP_TRY(hipMemsetAsync(x.d_probe, 0, (size_t)n_tiles * 16, cs()));          // (a wave that left no times shows)
        }
    }
    {
        ProfScope prof_scope;
        { const int rc_p = prof_scope.begin(); if (rc_p) return rc_p; }
        TileArgs a{p->P, p->fam.d_blob, d_packed, p->sample_kind, p->d_clips, p->d_norms, tiles, n_tiles, d_out, cs()};
        a.probe = probe ? x.d_probe : nullptr;
        if (fam_fast_launch(p, a)) return launch_failed(p);
    }
    if (probe) {
        HIP_TRY(hipMemcpyAsync(x.h_probe, x.d_probe, (size_t)n_tiles * 16, hipMemcpyDeviceToHost, cs()));
        HIP_TRY(hipEventRecord(x.probe_ev, cs()));
        std::copy(x.n_label, x.n_label + kXcdLabels, x.pending_n);
        x.probe_pending = true;
    }
    return PAA_OK;
}
static int fam_fast_execute(paa_plan *p, const void *d_packed, double *d_out, const Tile *tiles, long long n_tiles) {
    return fam_fast_execute_probe(p, d_packed, d_out, tiles, n_tiles, false);
}

// ---- kernels_ct.hpp: windows 2 RA RB (800, 640, 400, 320), any step / sample type / mode
static int fam_ct_select(const FamilyCtx &c, FamilyChoice &f, std::vector<unsigned char> &blob) {
    if (g_force_generic || !ct::ct_select(c.window, c.fs, c.tab->fft, c.mel(), c.chroma(), f.cl, blob)) return 0;
    f.lds = f.cl.lds; f.kernel_name = mode_kernel_name(c.mode, f.cl.name);
    return 1;
}
static void fam_ct_rule(FamilyCtx &c, RunRule &r) {
    // one wave per run, 4 frames per iteration; a run with t0 > 0 starts 1 frame early (2 with deltas) inside its first
    // iteration, so the first run of a clip gets `run` frames and the others run - halo: every run is whole iterations
    r.quantum = 4;
    r.halo_inside = (c.mode == 0) ? (c.deltas ? 2 : 1) : 0;
    r.run = choose_run_cap(c.p->clips, 4, 16, 256, 0, c.p->fam.cl.waves, c.num_cu(), r.halo_inside);
    r.fill_wg_runs = c.p->fam.cl.waves;          // (one workgroup per CU; A/B scripts/rounds/r05/gpu_r05aj.sh: -0.4 ... -2.0 % on the feature shapes)
}
static int fam_ct_launch(const paa_plan *p, const TileArgs &a) { return launch::ct(p->fam.cl, a); }

// ---- kernels_tri.hpp: three-pass register FFT -- the reference's default 50 ms windows at 48 / 44.1 kHz (2400, 2205), the
// 40 ms ones (1920, 1764), 1600, 1200, config 5's feature matrix (1102) and the odd 551 (50 ms at 11.025 kHz)
static int fam_tri_select(const FamilyCtx &c, FamilyChoice &f, std::vector<unsigned char> &blob) {
    if (g_force_generic || !tri::tri_select(c.window, c.mode, c.fs, c.mel(), c.chroma(), f.trl, blob)) return 0;
    f.lds = f.trl.lds; f.kernel_name = mode_kernel_name(c.mode, f.trl.name);
    return 1;
}
static void fam_tri_rule(FamilyCtx &c, RunRule &r) {
    // one wave per run, one frame per iteration; a run with t0 > 0 recomputes 1 frame (2 with deltas) first
    r.quantum = 1;
    r.run = choose_run_cap(c.p->clips, 1, 8, 96, (c.mode == 0) ? (c.deltas ? 2 : 1) : 0, c.p->fam.trl.waves, c.num_cu());
    // (balanced runs -- RunRule::fill_wg_runs = trl.waves -- were A/B-ed here too, scripts/rounds/r05/gpu_r05ad.sh: 3072 runs of 19 / 20
    // frames instead of 3000 of 20 for config 5 changed nothing beyond the noise, 0.3202 / 0.3184 ms: the equal runs stay)
}
static int fam_tri_launch(const paa_plan *p, const TileArgs &a) { return launch::tri(p->fam.trl, a); }

// ---- kernels_mix.hpp: in-place mixed-radix transform for every other length made of 2, 3, 5, 7, 11, 13
static int fam_mix_select(const FamilyCtx &c, FamilyChoice &f, std::vector<unsigned char> &blob) {
    if (g_force_generic || experiment_env("PAA_NO_MIX")) return 0;
    if (!mix::mix_layout(c.tab->fft, c.mel(), c.chroma(), c.F, f.ml, &blob)) return 0;
    f.lds = mix::mix_lds_bytes(f.ml);
    f.kernel_name = mode_kernel_name(c.mode, "mix");
    return 1;
}
static void fam_mix_rule(FamilyCtx &c, RunRule &r) {
    // one wave per run, one frame at a time (halo: 1 frame, 2 with deltas)
    r.quantum = 4;
    r.run = two_round_run(c.total_frames, c.p->fam.ml.waves, c.num_cu());
}
static int fam_mix_launch(const paa_plan *p, const TileArgs &a) { return launch::mix(p->fam.ml, a); }

// ---- kernels_blu.hpp: lengths with a prime factor above 13 (661, 1103, 736 ...): Bluestein's convolution on power-of-two transforms
static int fam_blu_select(const FamilyCtx &c, FamilyChoice &f, std::vector<unsigned char> &blob) {
    if (g_force_generic || experiment_env("PAA_NO_BLU")) return 0;
    if (!blu::blu_layout(c.tab->fft, c.mel(), c.chroma(), c.F, f.bl, &blob)) return 0;
    f.lds = blu::blu_lds_bytes(f.bl);
    f.kernel_name = mode_kernel_name(c.mode, "blu_" + std::to_string(1 << f.bl.log2m) + (f.bl.packed ? "p" : ""));
    return 1;
}
static void fam_blu_rule(FamilyCtx &c, RunRule &r) {
    // one wave per run, one frame at a time (halo: 1 frame, 2 with deltas)
    r.quantum = 4;
    r.run = two_round_run(c.total_frames, c.p->fam.bl.waves, c.num_cu());
}
static int fam_blu_launch(const paa_plan *p, const TileArgs &a) { return launch::blu(p->fam.bl, a); }

// ---- kernels_generic.hpp: Stockham passes in LDS (what no other one-wave family takes: tiny windows, prime factors above 13
// beyond 2730 samples), as long as the layout fits 160 KB of LDS
static int fam_generic_select(const FamilyCtx &c, FamilyChoice &f, std::vector<unsigned char> &blob) {
    generic_layout(c.tab->fft, c.mel(), c.chroma(), c.F, f.gl, &blob);
    f.lds = generic_lds_bytes(f.gl);
    if (f.lds > 160 * 1024) return 0;
    f.kernel_name = mode_kernel_name(c.mode, "generic");
    return 1;
}
static void fam_generic_rule(FamilyCtx &c, RunRule &r) {
    r.quantum = 4;
    r.run = two_round_run(c.total_frames, c.p->fam.gl.waves, c.num_cu());
}
static int fam_generic_launch(const paa_plan *p, const TileArgs &a) { return launch::generic(p->fam.gl, a); }

// ---- windows beyond the LDS envelope of the one-wave kernels --------------------------------------------------------------------
// kernels_wgr.hpp: the 1 s windows of music_thumbnailing at 16 / 8 kHz -- one fused launch, the transform in registers; its table
// (mel lane jobs + chroma lists) is the blob
static int fam_wgr_select(const FamilyCtx &c, FamilyChoice &f, std::vector<unsigned char> &blob) {
    const int id = wgr::wgr_shape_id(c.window);
    if (!id) return 0;
    wgr::WgrTab tab;
    if (!wgr::wgr_build_tab(wgr::wgr_threads(id), c.mel(), c.chroma(), tab)) return 0;   // (a mel bank its lane jobs cannot hold)
    blob.assign(reinterpret_cast<const unsigned char *>(&tab), reinterpret_cast<const unsigned char *>(&tab) + sizeof(tab));
    f.kernel_name = mode_kernel_name(c.mode, std::string("wgr_") + wgr::wgr_shape_name(id));
    return 1;
}
static int fam_wgr_work(FamilyCtx &c, std::vector<Tile> &runs) {
    wgr::wgr_build_runs(c.p->clips, g_num_cu, runs);          // runs of consecutive frames, about one per CU
    return PAA_OK;
}

// kernels_wgs.hpp / kernels_wg.hpp: the transform fits ONE WORKGROUP's LDS (split transforms: one radix-r0 pass straight from the
// samples, then one sub-transform at a time); the digit-reversal permutation is the blob of kernels_wg.hpp
static int wg_select(const FamilyCtx &c, FamilyChoice &f, std::vector<unsigned char> *perm_blob) {
    std::vector<unsigned short> perm;
    if (!wg::wg_layout(c.tab->fft, f.wl, perm)) return 0;
    if (perm_blob)
        perm_blob->assign(reinterpret_cast<const unsigned char *>(perm.data()), reinterpret_cast<const unsigned char *>(perm.data() + perm.size()));
    return 1;
}
// the real-input split on register passes (r0 x q samples: 44 100, 22 050, 48 000, 32 000, 24 000)
static int fam_wgs_select(const FamilyCtx &c, FamilyChoice &f, std::vector<unsigned char> &) {
    const wgs::Sel sel = wgs::wgs_select(c.window);
    if (!wg_select(c, f, nullptr) || !f.wl.r0 || !sel.r0) return 0;
    f.kernel_name = mode_kernel_name(c.mode, "wgs_" + std::to_string(sel.r0) + "x" + std::to_string(sel.q));
    return 1;
}
static int fam_wg_select(const FamilyCtx &c, FamilyChoice &f, std::vector<unsigned char> &blob) {
    if (!wg_select(c, f, &blob)) return 0;
    f.kernel_name = mode_kernel_name(c.mode, f.wl.r0 ? "wg_split_fft" : "wg_lds_fft");
    return 1;
}
// the frame list, cut in chunks whose spectrum rows fit the scratch, and the task lists of the split transforms (wgs_r0: the
// register split of kernels_wgs.hpp, else kernels_wg.hpp's)
static int wg_build_work(paa_plan *p, int wgs_r0) {
    // spectrum scratch: one row of Nf doubles per frame of a chunk, at most 1 GiB; a chunk that starts inside a clip
    // begins with that clip's previous frame once more (halo: only its spectrum row is wanted)
    const long long cap = wg_chunk_frames(p->P.Nf);
    long long first = 0;
    for (size_t c = 0; c < p->clips.size(); ++c)
        for (long long t = 0; t < p->clips[c].T; ++t) {
            long long in_chunk = (long long)p->wg_frames.size() - first;
            if (in_chunk >= cap) {
                p->wg_chunks.emplace_back(first, (long long)p->wg_frames.size());
                first = (long long)p->wg_frames.size();
                in_chunk = 0;
                if (t > 0 && p->mode != 1) p->wg_frames.push_back(wg::FrameRef{(int)c, (int)(t - 1), 0, 1});
            }
            p->wg_frames.push_back(wg::FrameRef{(int)c, (int)t, (int)((long long)p->wg_frames.size() - first), 0});
        }
    if ((long long)p->wg_frames.size() > first) p->wg_chunks.emplace_back(first, (long long)p->wg_frames.size());
    for (auto &ch : p->wg_chunks) {
        p->wg_rows = std::max(p->wg_rows, ch.second - ch.first);
        for (long long i = ch.first; i < ch.second; ++i) p->wg_frames[(size_t)i].row = (int)(i - ch.first);
    }
    int rc = upload_pooled(&p->d_wg_frames, p->wg_frames.data(), std::max<size_t>(p->wg_frames.size(), 1));
    if (rc) return rc;
    if (wgs_r0) {
        // the tasks of a frame side by side (FrameRef::halo = halo | type << 8)
        const int n_types = wgs::wgs_task_types(wgs_r0);
        for (auto &ch : p->wg_chunks) {
            const long long t0 = (long long)p->wg_tasks.size();
            auto push = [&](long long i, int ty) {
                wg::FrameRef f = p->wg_frames[(size_t)i];
                f.halo |= ty << 8;
                p->wg_tasks.push_back(f);
            };
            if (wgs_r0 == 6) {
                // three sub-transforms per frame: {1, 2} and the packed one -- the packed units of two CONSECUTIVE frames of a clip (consecutive
                // rows) share a task (type 1, on the first frame's record); a frame without such a partner runs its packed unit alone (type 2)
                for (long long i = ch.first; i < ch.second;) {
                    const wg::FrameRef &a = p->wg_frames[(size_t)i];
                    const bool pair = i + 1 < ch.second && p->wg_frames[(size_t)i + 1].clip == a.clip && p->wg_frames[(size_t)i + 1].t == a.t + 1 &&
                                      p->wg_frames[(size_t)i + 1].row == a.row + 1;
                    push(i, 0);
                    if (pair) { push(i + 1, 0); push(i, 1); i += 2; }
                    else { push(i, 2); i += 1; }
                }
            } else {
                for (long long i = ch.first; i < ch.second; ++i)
                    for (int ty = 0; ty < n_types; ++ty) push(i, ty);
            }
            p->wg_task_chunks.emplace_back(t0, (long long)p->wg_tasks.size());
        }
    } else if (p->fam.wl.r0) {
        // tasks of a frame: sub-transform 0 alone, the pairs {q, r0 - q}, r0 / 2 alone (FrameRef::halo = halo | q << 8)
        const int r0 = p->fam.wl.r0;
        for (auto &ch : p->wg_chunks) {
            const long long t0 = (long long)p->wg_tasks.size();
            // (the pairs first: they cost twice what the single sub-transforms do, and tasks are handed out in list order)
            for (int pairs = 1; pairs >= 0; --pairs)
                for (long long i = ch.first; i < ch.second; ++i)
                    for (int q = 0; 2 * q <= r0; ++q) {
                        if ((q != 0 && 2 * q != r0) != (pairs != 0)) continue;
                        wg::FrameRef f = p->wg_frames[(size_t)i];
                        f.halo |= q << 8;
                        p->wg_tasks.push_back(f);
                    }
            p->wg_task_chunks.emplace_back(t0, (long long)p->wg_tasks.size());
        }
    } else {
        return PAA_OK;
    }
    if (p->wg_tasks.size() > 0x7fffffffULL) return fail(PAA_ERR_UNSUPPORTED, "too many frames for the split transform");
    return upload_pooled(&p->d_wg_tasks, p->wg_tasks.data(), std::max<size_t>(p->wg_tasks.size(), 1));
}
static int fam_wgs_work(FamilyCtx &c, std::vector<Tile> &) { return wg_build_work(c.p, wgs::wgs_select(c.window).r0); }
static int fam_wg_work(FamilyCtx &c, std::vector<Tile> &) { return wg_build_work(c.p, 0); }
// one WgArgs per execute of a workgroup-wide family
static WgArgs wg_args(const paa_plan *p, const void *d_packed, double *d_out) {
    return WgArgs{p->P, d_packed, p->sample_kind, p->d_clips, p->d_norms, d_out, g_num_cu, cs()};
}
static int fam_wgr_execute(paa_plan *p, const void *d_packed, double *d_out, const Tile *runs, long long n_runs) {
    return run_wgr(p, wg_args(p, d_packed, d_out), runs, n_runs);
}
static int fam_wgs_execute(paa_plan *p, const void *d_packed, double *d_out, const Tile *, long long) {
    return run_wgs(p, wg_args(p, d_packed, d_out), wgs::wgs_select(p->P.W));
}
static int fam_wg_execute(paa_plan *p, const void *d_packed, double *d_out, const Tile *, long long) {
    const WgArgs a = wg_args(p, d_packed, d_out);
    return with_sample_type(p->sample_kind, [&](auto tag) {
        typedef PAA_SAMPLE_T(tag) T;
        wg_kernel_order<T>();
        return p->fam.wl.r0 ? run_wg_split<T>(p, a) : run_wg_lds<T>(p, a);
    });
}

// kernels_big.hpp: chunked Stockham passes through HBM scratch (what nothing else takes; no CPU fallback)
static int fam_hbm_select(const FamilyCtx &, FamilyChoice &f, std::vector<unsigned char> &) {
    f.kernel_name = "big_window_hbm_passes";
    return 1;
}
static int no_work(FamilyCtx &, std::vector<Tile> &) { return PAA_OK; }
static int fam_hbm_execute(paa_plan *p, const void *d_packed, double *d_out, const Tile *, long long) {
    return with_sample_type(p->sample_kind, [&](auto tag) { return run_big<PAA_SAMPLE_T(tag)>(p, d_packed, d_out); });
}

// in choice order; ranged / norms_inline: the one-wave families only
static const Family kFamilies[] = {
    {"fast", fam_fast_select, tile_work<fam_fast_rule>, fam_fast_execute, true, true},
    {"ct", fam_ct_select, tile_work<fam_ct_rule>, tile_execute<fam_ct_launch>, true, true},
    {"tri", fam_tri_select, tile_work<fam_tri_rule>, tile_execute<fam_tri_launch>, true, true},
    {"mix", fam_mix_select, tile_work<fam_mix_rule>, tile_execute<fam_mix_launch>, true, true},
    {"blu", fam_blu_select, tile_work<fam_blu_rule>, tile_execute<fam_blu_launch>, true, true},
    {"generic", fam_generic_select, tile_work<fam_generic_rule>, tile_execute<fam_generic_launch>, true, true},
    {"wgr", fam_wgr_select, fam_wgr_work, fam_wgr_execute, false, false},
    {"wgs", fam_wgs_select, fam_wgs_work, fam_wgs_execute, false, false},
    {"wg", fam_wg_select, fam_wg_work, fam_wg_execute, false, false},
    {"hbm", fam_hbm_select, no_work, fam_hbm_execute, false, false},
};
constexpr int kNumFamilies = (int)(sizeof(kFamilies) / sizeof(kFamilies[0]));

static void free_family_choices(TableSet &t) {
    for (auto &kv : t.choices)
        if (kv.second && kv.second->d_blob) pool_free(kv.second->d_blob);
    t.choices.clear();
}

// the first entry of kFamilies that takes the shape -> c.p->fam.  The choice is kept with the table set of (fs, window): the next
// plan of the same (mode, rows) copies it back instead of rebuilding the layout and uploading the table blob again
static int choose_family(FamilyCtx &c) {
    paa_plan *p = c.p;
    // the fast family looks at (step, sample type) too; nobody else does
    const int fast_key = (c.mode == 0 && c.window == 800 && c.sample_kind == 0 && (c.step == 400 || c.step == 800)) ? c.step : 0;
    const auto key = std::make_tuple(c.mode, c.F, fast_key);
#ifndef PAA_EXPERIMENTS          // (experiment switches change the choice from plan to plan: no cache in those builds)
    auto it = c.tab->choices.find(key);
    if (it != c.tab->choices.end() && !g_force_generic) {
        p->fam = *it->second;
        p->blob_cached = true;
        return PAA_OK;
    }
#endif
    for (int i = 0; i < kNumFamilies; ++i) {
        std::vector<unsigned char> blob;
        p->fam = FamilyChoice();
        int rc = kFamilies[i].select(c, p->fam, blob);
        if (rc < 0) return rc;
        if (rc == 0) continue;
        p->fam.family = i;
        if (!blob.empty() && (rc = upload_pooled(&p->fam.d_blob, blob.data(), blob.size()))) return rc;
#ifndef PAA_EXPERIMENTS
        if (!g_force_generic) {
            c.tab->choices[key] = std::make_shared<FamilyChoice>(p->fam);      // (the blob now belongs to the table set)
            p->blob_cached = true;
        }
#endif
        return PAA_OK;
    }
    return fail(PAA_ERR_UNSUPPORTED, "no kernel family takes window %d", c.window);
}
