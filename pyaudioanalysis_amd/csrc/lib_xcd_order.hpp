// Which XCD is slow: calibration of the 800-sample kernel's run placement.  One of the units paa_lib.hip is made of (included by
// lib_plan.hpp in front of the plan structure).
//
// A one-round launch of the one-workgroup-per-CU kernel ends when its slowest XCD has finished its largest SIMD total, and the
// eight XCDs of an MI355X differ by a few percent in sustained clock.  balanced_runs (lib_plan.hpp) cuts
// a plan into runs of two lengths; with an order of the eight labels (label = workgroup mod 8: the workgroups of a label share an
// XCD) it deals the short ones to the slowest labels.  The order is measured: every now and then an execute of such a plan is a
// PROBE launch (kernels_fast.hpp: TabLayout::probe), whose per-wave entry / exit times come back through pinned memory and are
// folded in by a LATER execute, once the copy's event is complete -- no execute waits for a probe.
#pragma once

constexpr int kXcdLabels = 8;
constexpr int kXcdFirstProbes = 8;          // probe launches at the start of a device's life, then ...
constexpr int kXcdProbeEvery = 256;         // ... one execute in this many
constexpr double kXcdAvg = 0.25;            // weight of a new probe in the averaged time per iteration
// two labels change places only when their averages differ by more than this fraction: one launch's label times scatter by about
// +- 1 % (profiles/r13_fast800_xcd_order_probe.txt), the average of a few by half of that, and a difference below it is worth
// less than that to the launch
constexpr double kXcdMargin = 0.005;
constexpr unsigned long long kXcdTimeMask = (1ULL << 60) - 1;          // a probe's exit word: XCC id above, 100 MHz counter below

// per device (one process drives one device; paa_shutdown resets it).  Guarded by its own mutex, like the block pool: plans of
// several lanes consult it
struct XcdCal {
    std::mutex mu;
    bool off = false;                       // the device does not map label -> XCD the way the placement assumes: no probes, no order
    bool forced = false;                    // paa_debug_xcd_force_order: `order` is the caller's, probes do not move it
    bool have_order = false;
    int order[kXcdLabels] = {0, 1, 2, 3, 4, 5, 6, 7};         // labels, slowest first
    bool kept_have = false;                 // the measured order a forced one replaced: back in force when the forced one is cleared
    int kept[kXcdLabels] = {0, 1, 2, 3, 4, 5, 6, 7};
    unsigned long long epoch = 0;           // bumped whenever the order in force changes; 0: there has never been one
    double tau[kXcdLabels] = {0, 0, 0, 0, 0, 0, 0, 0};        // averaged ticks per iteration of a label's slowest SIMD
    long long folded = 0;                   // probes in the average
    int cand[kXcdLabels] = {0, 1, 2, 3, 4, 5, 6, 7};          // a new order seen by the last probe (cand_seen), not yet in force
    int cand_seen = 0;
    long long executes = 0, probes = 0;     // executes of balanced plans / probe launches among them
};
static XcdCal g_xcd;

// PAA_XCD_ORDER=0: no probes, no order -- the even spread of balanced_runs, whatever was measured or forced
static bool xcd_enabled() {
    const char *e = getenv("PAA_XCD_ORDER");
    return !(e && e[0] == '0');
}
static void xcd_reset() {
    std::lock_guard<std::mutex> lk(g_xcd.mu);
    g_xcd.off = g_xcd.forced = g_xcd.have_order = g_xcd.kept_have = false;
    g_xcd.epoch = 0;
    g_xcd.folded = 0;
    g_xcd.cand_seen = 0;
    g_xcd.executes = g_xcd.probes = 0;
    for (int i = 0; i < kXcdLabels; ++i) { g_xcd.order[i] = g_xcd.cand[i] = i; g_xcd.tau[i] = 0.0; }
}
// the order in force (false: none -- the even spread) and its epoch
static bool xcd_current(int *order8, unsigned long long *epoch) {
    std::lock_guard<std::mutex> lk(g_xcd.mu);
    const bool on = xcd_enabled() && !g_xcd.off && (g_xcd.forced || g_xcd.have_order);
    *epoch = on ? g_xcd.epoch : 0;
    if (on) std::copy(g_xcd.order, g_xcd.order + kXcdLabels, order8);
    return on;
}
// counts an execute of a balanced plan; is it a probe launch?  can_probe: the plan can take one now (its last record has been
// read, its kernel instance carries the probe) -- an opening probe that cannot be taken waits for the next execute
static bool xcd_want_probe(bool can_probe) {
    std::lock_guard<std::mutex> lk(g_xcd.mu);
    const long long k = g_xcd.executes++;
    if (g_xcd.off || !can_probe) return false;
    if (!(g_xcd.probes < kXcdFirstProbes || k % kXcdProbeEvery == 0)) return false;
    ++g_xcd.probes;
    return true;
}

// the largest SIMD total (iterations of the waves that share a SIMD) of every label in a tile list of wg_runs tiles per workgroup;
// a tile with t0 > 0 holds `shrink` halo frames inside its first iteration
static void xcd_label_totals(const Tile *tiles, long long n_tiles, int wg_runs, int quantum, int shrink, int *n_label) {
    std::fill(n_label, n_label + kXcdLabels, 0);
    for (long long first = 0; first < n_tiles; first += wg_runs) {
        int simd[4] = {0, 0, 0, 0};
        for (long long i = first; i < std::min<long long>(first + wg_runs, n_tiles); ++i)
            simd[(i - first) % 4] += (tiles[i].cnt + (tiles[i].t0 > 0 ? shrink : 0) + quantum - 1) / quantum;
        int &n = n_label[(first / wg_runs) % kXcdLabels];
        for (int s = 0; s < 4; ++s) n = std::max(n, simd[s]);
    }
}

// What one probe record says.  rec: two words per tile (entry; exit | XCC id << 60); n_label: xcd_label_totals of the list the
// launch used.  t_label: end of each label's last wave, in ticks after the launch's first wave entered; xcc_label: the XCC id
// its waves ran on.  Returns 1: a usable record; 0: an incomplete one (a wave without times); -1: the device maps differently (a grid
// that is not num_cu workgroups with num_cu a multiple of 8, or a label on more than one XCD).  The GRID counts, not the tiles: a
// plan of several clips may have a few runs fewer than wave slots (balanced_runs: given <= slots), its last workgroup is then short
static int xcd_read_record(const unsigned long long *rec, long long n_tiles, int wg_runs, int num_cu, long long *t_label, int *xcc_label) {
    if (num_cu % kXcdLabels != 0 || wg_runs < 1 || (n_tiles + wg_runs - 1) / wg_runs != (long long)num_cu) return -1;
    unsigned long long first = ~0ULL;
    for (long long i = 0; i < n_tiles; ++i) {
        const unsigned long long in = rec[2 * i], out = rec[2 * i + 1] & kXcdTimeMask;
        if (in == 0 || out <= in) return 0;
        first = std::min(first, in);
    }
    std::fill(t_label, t_label + kXcdLabels, 0LL);
    std::fill(xcc_label, xcc_label + kXcdLabels, -1);
    for (long long i = 0; i < n_tiles; ++i) {
        const int label = (int)((i / wg_runs) % kXcdLabels), xcc = (int)(rec[2 * i + 1] >> 60);
        if (xcc_label[label] >= 0 && xcc_label[label] != xcc) return -1;
        xcc_label[label] = xcc;
        t_label[label] = std::max<long long>(t_label[label], (long long)((rec[2 * i + 1] & kXcdTimeMask) - first));
    }
    return 1;
}

// labels by averaged time per iteration, slowest first, starting from `from`: a label moves in front of its neighbour only when
// it is slower by more than kXcdMargin, so labels the probes cannot tell apart keep their places from probe to probe
static void xcd_sort(const double *tau, const int *from, int *order8) {
    std::copy(from, from + kXcdLabels, order8);
    for (int i = 1; i < kXcdLabels; ++i)
        for (int j = i; j > 0 && tau[order8[j]] > tau[order8[j - 1]] * (1.0 + kXcdMargin); --j) std::swap(order8[j], order8[j - 1]);
}

// folds one probe record into the device's averages; the order in force follows once the same new order came out of two
// consecutive probes
static void xcd_fold(const unsigned long long *rec, long long n_tiles, int wg_runs, int num_cu, const int *n_label) {
    long long t_label[kXcdLabels];
    int xcc_label[kXcdLabels];
    const int ok = xcd_read_record(rec, n_tiles, wg_runs, num_cu, t_label, xcc_label);
    std::lock_guard<std::mutex> lk(g_xcd.mu);
    if (ok < 0) { g_xcd.off = true; return; }
    if (ok == 0 || g_xcd.off) return;
    for (int l = 0; l < kXcdLabels; ++l)
        if (n_label[l] < 1) return;
    for (int l = 0; l < kXcdLabels; ++l) {
        const double t = (double)t_label[l] / (double)n_label[l];
        g_xcd.tau[l] = g_xcd.folded ? (1.0 - kXcdAvg) * g_xcd.tau[l] + kXcdAvg * t : t;
    }
    ++g_xcd.folded;
    if (g_xcd.forced) return;
    // (sorted from the order the last probe proposed, if it proposed one: labels within the margin keep the places they had there)
    int now[kXcdLabels];
    xcd_sort(g_xcd.tau, g_xcd.cand_seen > 0 ? g_xcd.cand : g_xcd.order, now);
    if (g_xcd.have_order && std::equal(now, now + kXcdLabels, g_xcd.order)) { g_xcd.cand_seen = 0; return; }
    if (g_xcd.cand_seen > 0 && std::equal(now, now + kXcdLabels, g_xcd.cand)) {
        std::copy(now, now + kXcdLabels, g_xcd.order);
        g_xcd.have_order = true;
        g_xcd.cand_seen = 0;
        ++g_xcd.epoch;
        return;
    }
    std::copy(now, now + kXcdLabels, g_xcd.cand);
    g_xcd.cand_seen = 1;
}

// what a plan keeps for it (paa_plan::xcd)
struct XcdPlan {
    bool balanced = false;                  // the tile list is balanced_runs' (fast family, one range)
    bool resident = false;                  // a plan of paa_plan_create: it lives across executes -- it probes and re-cuts; the per-call
                                            // plans of the host-buffer entry points are only CUT under the order in force
    int run = 0, quantum = 0, shrink = 0, wg_runs = 0, min_run = 0;      // the RunRule its list was cut by
    unsigned long long epoch = 0;           // epoch of the order its list was cut under (0: the even spread)
    int n_label[kXcdLabels] = {0, 0, 0, 0, 0, 0, 0, 0};                  // xcd_label_totals of the list
    std::vector<Tile> tiles;                // host copy of the list (resident plans)
    unsigned long long *d_probe = nullptr;  // 2 words per tile
    unsigned long long *h_probe = nullptr;  // pinned: a probe launch's record
    Tile *h_tiles = nullptr;                // pinned: staging of a re-cut list
    hipEvent_t probe_ev = nullptr, upload_ev = nullptr;
    bool probe_pending = false, upload_pending = false;
    int pending_n[kXcdLabels] = {0, 0, 0, 0, 0, 0, 0, 0};                // n_label of the list the pending probe ran on
};
static void xcd_plan_free(XcdPlan &x) {
    if (x.probe_ev) (void)hipEventDestroy(x.probe_ev);
    if (x.upload_ev) (void)hipEventDestroy(x.upload_ev);
    if (x.h_probe) (void)hipHostFree(x.h_probe);
    if (x.h_tiles) (void)hipHostFree(x.h_tiles);
    x.probe_ev = x.upload_ev = nullptr;
    x.h_probe = nullptr;
    x.h_tiles = nullptr;
}
