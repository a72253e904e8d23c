// The 2 RA RB register-FFT family (kernels_ct.hpp: windows 800, 640, 400, 320) -- own translation unit, see family_launch.hpp.
#include <cstdlib>
#include <cstring>

#include "family_launch.hpp"

namespace paa {
namespace launch {

template <typename SH, typename T, int MODE, int DELTAS>
static int ct_one(const ct::CtLaunch &cl, const TileArgs &a) {
    static LdsAttrCache attr;
    return tile_launch(&ct::st_ct_kernel<SH, T, MODE, DELTAS, 8>, attr, 8, cl.lds, cl.layout, a);
}
template <typename SH, typename T>
static int ct_mode(const ct::CtLaunch &cl, const TileArgs &a) {
    if (a.P.mode == 1) return ct_one<SH, T, 1, 0>(cl, a);
    if (a.P.mode == 2) return ct_one<SH, T, 2, 0>(cl, a);
    return a.P.deltas ? ct_one<SH, T, 0, 1>(cl, a) : ct_one<SH, T, 0, 0>(cl, a);
}
template <typename T>
static int ct_shape(const ct::CtLaunch &cl, const TileArgs &a) {
    switch (cl.shape) {
        case 0: return ct_mode<ct::S800, T>(cl, a);
        case 1: return ct_mode<ct::S640, T>(cl, a);
        case 2: return ct_mode<ct::S320, T>(cl, a);
        case 3: return ct_mode<ct::S400, T>(cl, a);
        default: return -1;
    }
}
int ct(const ct::CtLaunch &cl, const TileArgs &a) {
    return with_sample_type(a.sample_kind, [&](auto tag) { return ct_shape<PAA_SAMPLE_T(tag)>(cl, a); });
}

PAA_PHASE_READER(phase_ct)
}  // namespace launch
}  // namespace paa
