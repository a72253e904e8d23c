// Three-pass register FFT (kernels_tri.hpp), first unit: the 50 ms windows at 48 / 44.1 kHz and config 5's feature matrix
// (2400, 2205, 1102) -- see family_launch.hpp.
#define PAA_TRI_SHAPES_HERE(X) X(0, S2400) X(1, S2205) X(7, S1102)
#include <cstdlib>
#include <cstring>

#include "family_tri_launch.hpp"

namespace paa {
namespace launch {
int tri_part_a(const tri::TriLaunch &tl, const TileArgs &a) { return tri_here(tl, a); }
// which unit holds a shape (tri_shape_of's numbering)
int tri(const tri::TriLaunch &tl, const TileArgs &a) {
    const bool here = tl.shape == 0 || tl.shape == 1 || tl.shape == 7;
    if (tl.shape >= 8) return tri_part_c(tl, a);
    return here ? tri_part_a(tl, a) : tri_part_b(tl, a);
}
PAA_PHASE_READER(phase_tri_a)
}  // namespace launch
}  // namespace paa
