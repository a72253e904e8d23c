// The workgroup-wide three-pass register transform with fused features (kernels_wgr.hpp: 16 000- and 8 000-sample windows) -- own
// translation unit, see family_launch.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "family_launch.hpp"
#include "kernels_wgr.hpp"

namespace paa {
namespace launch {

template <typename SH, typename T, int MODE>
static int wgr_one(const Tile *runs, long long n_runs, const wgr::WgrTab *d_tab, const WgArgs &a) {
    static LdsAttrCache attr;
    const unsigned grid = (unsigned)std::min<long long>(n_runs, a.num_cu);
    return wg_launch(&wgr::wgr_kernel<SH, T, MODE>, attr, grid, SH::NT, (size_t)SH::LDS_BYTES, a.stream, a.P, (const T *)a.d_packed, a.clips,
                     a.norms, runs, (int)n_runs, d_tab, a.d_out);
}
template <typename SH>
static int wgr_shape(int mode, const Tile *runs, long long n_runs, const wgr::WgrTab *d_tab, const WgArgs &a) {
    return with_sample_type(a.sample_kind, [&](auto tag) {
        typedef PAA_SAMPLE_T(tag) T;
        if (mode == 0) return wgr_one<SH, T, 0>(runs, n_runs, d_tab, a);
        if (mode == 1) return wgr_one<SH, T, 1>(runs, n_runs, d_tab, a);
        return wgr_one<SH, T, 2>(runs, n_runs, d_tab, a);
    });
}
int wgr(int shape_id, int mode, const Tile *runs, long long n_runs, const wgr::WgrTab *d_tab, const WgArgs &a) {
    if (shape_id == 1) return wgr_shape<wgr::S16000>(mode, runs, n_runs, d_tab, a);
    if (shape_id == 2) return wgr_shape<wgr::S8000>(mode, runs, n_runs, d_tab, a);
    return -1;
}

PAA_PHASE_READER(phase_wgr)
}  // namespace launch
}  // namespace paa
