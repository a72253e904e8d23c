// Host ladder of the three-pass register FFT (kernels_tri.hpp), included by the three family_tri_*.hip units and by nothing
// else: each of them names the shapes it instantiates in PAA_TRI_SHAPES_HERE before the include.  (Internal linkage: the
// same ladder over different shapes in every unit.)
#pragma once
#include "family_launch.hpp"

namespace paa {
namespace launch {

template <typename SH, typename T, int MODE, int DELTAS>
static int tri_one(const tri::TriLaunch &tl, const TileArgs &a) {
    static LdsAttrCache attr;
    // (tl.waves <= the shape's maximum, which is what __launch_bounds__ promises)
    return tile_launch(&tri::st_tri_kernel<SH, T, MODE, DELTAS>, attr, tl.waves, tl.lds, tl.layout, a);
}
template <typename SH, typename T>
static int tri_mode(const tri::TriLaunch &tl, const TileArgs &a) {
    if (a.P.mode == 1) return tri_one<SH, T, 1, 0>(tl, a);
    if (a.P.mode == 2) return tri_one<SH, T, 2, 0>(tl, a);
    return a.P.deltas ? tri_one<SH, T, 0, 1>(tl, a) : tri_one<SH, T, 0, 0>(tl, a);
}
template <typename T>
static int tri_shape(const tri::TriLaunch &tl, const TileArgs &a) {
    switch (tl.shape) {
#define PAA_TRI_GO(ID, SH) case ID: return tri_mode<tri::SH, T>(tl, a);
        PAA_TRI_SHAPES_HERE(PAA_TRI_GO)
#undef PAA_TRI_GO
        default: return -1;
    }
}
static int tri_here(const tri::TriLaunch &tl, const TileArgs &a) {
    return with_sample_type(a.sample_kind, [&](auto tag) { return tri_shape<PAA_SAMPLE_T(tag)>(tl, a); });
}

}  // namespace launch
}  // namespace paa
