// The 800-sample int16 kernels (kernels_fast.hpp) -- own translation unit, see family_launch.hpp.
#include <cstdlib>
#include <cstring>

#include "family_launch.hpp"

namespace paa {
namespace launch {

template <int S, int DELTAS, int FIXED, int NW>
static int fast_one(const FastLaunch &fl, const TileArgs &a) {
    static LdsAttrCache attr;
    f800::TabLayout layout = fl.layout;
    layout.probe = FIXED ? a.probe : nullptr;          // a calibration launch (lib_xcd_order.hpp), else null
    return tile_launch(&f800::st_fast_800_kernel<S, DELTAS, FIXED, NW>, attr, NW, fl.lds, layout, a);
}
template <int S, int NW>
static int fast_step(const FastLaunch &fl, const TileArgs &a) {
    if (fl.layout.fixed_lists) return a.P.deltas ? fast_one<S, 1, 1, NW>(fl, a) : fast_one<S, 0, 1, NW>(fl, a);
    return a.P.deltas ? fast_one<S, 1, 0, NW>(fl, a) : fast_one<S, 0, 0, NW>(fl, a);
}
int fast(const FastLaunch &fl, const TileArgs &a) {
    if (!a.blob) return -1;
    if (fl.variant == 800 && fl.waves_per_cu == 8) return fast_step<400, 8>(fl, a);
    if (fl.variant == 1600 && fl.waves_per_cu == 8) return fast_step<800, 8>(fl, a);
#ifdef PAA_EXPERIMENTS      // the one-wave-per-SIMD instances (NW = 4, ~340 registers) are the A/B baseline of scripts/ab_waves.sh
    if (fl.variant == 800) return fast_step<400, 4>(fl, a);
    if (fl.variant == 1600) return fast_step<800, 4>(fl, a);
#endif
    return -1;
}

PAA_PHASE_READER(phase_fast)
}  // namespace launch
}  // namespace paa
