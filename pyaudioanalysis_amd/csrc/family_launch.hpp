// Launch entry points of the feature-kernel families.  Every family is its own translation unit (family_<name>.hip: its
// kernels AND the host ladder that picks an instance are there and nowhere else, so the families compile in parallel); the
// host side of the library (paa_lib.hip and the lib_*.hpp units it is made of) sees only these functions and the families'
// host-side layout / selection code in the kernel headers.  All of them queue ONE kernel on `stream` and return 0, or -1 when
// the launch failed (hipGetLastError has the reason).  The one-wave families (fast, ct, tri, mix, blu, generic) take their
// layout and one TileArgs record, and launch through tile_launch below; the workgroup-wide ones (wgr, wgs here, the wg kernels
// of lib_plan.hpp) take one WgArgs record plus what is their own, and launch through wg_launch.  Both helpers keep ONE rule
// for kernels with more than 64 KB of LDS: one LdsAttrCache per kernel instance, raised to exactly the bytes launched.
// The model families (svc, svr, knn, forest, hmm, diar, lda) have model_launch.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_ct.hpp"
#include "kernels_fast.hpp"
#include "kernels_generic.hpp"
#include "kernels_mix.hpp"
#include "kernels_tri.hpp"
#include "kernels_blu.hpp"

namespace paa {
// what every launch of a one-wave family over a tile list needs (lib_dispatch.hpp: tile_execute fills it from the plan)
struct TileArgs {
    const PlanDev &P;
    const unsigned char *blob;       // the family's device tables
    const void *d_packed;            // the samples; sample_kind: 0 int16, 1 float64, 2 interleaved stereo int16 (summed in the kernels' loads)
    int sample_kind;
    const ClipDev *clips;
    const ClipNorm *norms;
    const Tile *tiles;
    long long n_tiles;
    double *d_out;
    hipStream_t stream;
    unsigned long long *probe = nullptr;      // fast family, calibration launches: two words per tile (kernels_fast.hpp: TabLayout::probe)
};
// the launch of every one-wave family: `waves` tiles per workgroup, one wave each.  `attr` is the cache of THIS kernel
// instance (a static of the caller, which is a template over the instance); the attribute is raised to exactly `lds`
// bytes, again after paa_shutdown -> paa_init (LdsAttrCache's generation)
template <typename L, typename T>
int tile_launch(void (*kernel)(PlanDev, L, const unsigned char *, const T *, const ClipDev *, const ClipNorm *, const Tile *, int, double *),
                LdsAttrCache &attr, int waves, size_t lds, const L &layout, const TileArgs &a) {
    if (!attr.covers(lds)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return -1;
        attr.set(lds);
    }
    const unsigned grid = (unsigned)((a.n_tiles + waves - 1) / waves);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * waves), lds, a.stream, a.P, layout, a.blob, (const T *)a.d_packed, a.clips, a.norms,
                       a.tiles, (int)a.n_tiles, a.d_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// what every launch of a workgroup-wide family needs (lib_dispatch.hpp: wg_args fills it from the plan)
struct WgArgs {
    const PlanDev &P;
    const void *d_packed;            // the samples, as TileArgs::d_packed
    int sample_kind;
    const ClipDev *clips;
    const ClipNorm *norms;
    double *d_out;
    int num_cu;
    hipStream_t stream;
};
// the scratch rows of a chunk of frames between a spectrum kernel and its feature kernel (lib_plan.hpp: wg_scratch): Nf magnitudes
// and 3 time-domain partials per row; psum: kernels_wgs.hpp's partial sums, 4 doubles per row and unit
struct WgScratch {
    double *spec, *tfeat, *psum;
};
// the launch of every workgroup-wide kernel, under tile_launch's rule for `attr`
template <typename... Params, typename... Args>
int wg_launch(void (*kernel)(Params...), LdsAttrCache &attr, unsigned grid, unsigned threads, size_t lds, hipStream_t stream,
              const Args &...args) {
    if (!attr.covers(lds)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return -1;
        attr.set(lds);
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, stream, args...);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

namespace wgr { struct WgrTab; }
namespace launch {

// kernels_fast.hpp: window 800, step 400 / 800, int16 (a.blob: FastTables::d_blob)
int fast(const FastLaunch &fl, const TileArgs &a);
// kernels_ct.hpp: windows 2 RA RB (800, 640, 400, 320)
int ct(const ct::CtLaunch &cl, const TileArgs &a);
// kernels_tri.hpp: three-pass register FFT (2400, 2205, 1764, 1920, 1600, 1200, 1102 features, 551; 1024, 2048, 512); three units
int tri(const tri::TriLaunch &tl, const TileArgs &a);
int tri_part_a(const tri::TriLaunch &tl, const TileArgs &a);
int tri_part_b(const tri::TriLaunch &tl, const TileArgs &a);
int tri_part_c(const tri::TriLaunch &tl, const TileArgs &a);
// kernels_mix.hpp: in-place mixed-radix transform (every other length made of 2, 3, 5, 7, 11, 13)
int mix(const mix::MixLayout &ml, const TileArgs &a);
// kernels_blu.hpp: Bluestein convolution on power-of-two transforms (lengths with a prime factor above 13)
int blu(const blu::BluLayout &bl, const TileArgs &a);
// kernels_generic.hpp: Stockham passes in LDS (what is left)
int generic(const GenLayout &gl, const TileArgs &a);
// kernels_wgr.hpp: workgroup-wide three-pass register transform with fused features (16 000- / 8 000-sample windows); `runs`:
// runs of consecutive frames, one workgroup walks runs b, b + grid, ...
int wgr(int shape_id, int mode, const Tile *runs, long long n_runs, const wgr::WgrTab *d_tab, const WgArgs &a);
// kernels_wgs.hpp: real-input split of the long even windows r0 x q samples (12 / 6 x 3675: 44 100, 22 050; 12 / 8 / 6 x 4000: 48 000, 32 000, 24 000),
// three register passes per sub-transform; `tasks`: (frame, task type) records handed out through `counter` (zero at the first launch; the kernel
// leaves it at zero); magnitudes go to the frames' UNIT-MAJOR rows of s.spec (spectrogram plans: d_out, natural order), the time-domain partials of
// a frame to s.tfeat, the units' sum X / sum (k + 1) X / max X to s.psum (r0 / 2 units)
int wgs(int r0, int q, const wg::FrameRef *tasks, int n_tasks, int *counter, const WgScratch &s, const WgArgs &a);
// ... and the features of those frames from the unit-major rows (one workgroup per frame)
int wgs_feat(int r0, int q, const wg::FrameRef *frames, int n_frames, const WgScratch &s, const WgArgs &a);

// timing builds (-DPAA_F800_TIMING / _TRACE): per-unit readers of the kernels' phase-cycle counters (kernels_fast.hpp:
// PAA_PHASE_READER); no-ops otherwise
int phase_fast(unsigned long long *acc16, unsigned long long *trace, int max_waves);
int phase_ct(unsigned long long *acc16, unsigned long long *trace, int max_waves);
int phase_tri_a(unsigned long long *acc16, unsigned long long *trace, int max_waves);
int phase_tri_b(unsigned long long *acc16, unsigned long long *trace, int max_waves);
int phase_tri_c(unsigned long long *acc16, unsigned long long *trace, int max_waves);
int phase_rmg(unsigned long long *acc16, unsigned long long *trace, int max_waves);
int phase_blu(unsigned long long *acc16, unsigned long long *trace, int max_waves);
int phase_wgr(unsigned long long *acc16, unsigned long long *trace, int max_waves);

}  // namespace launch
}  // namespace paa
