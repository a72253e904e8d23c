// Three-pass register FFT (kernels_tri.hpp), third unit: the power-of-two windows 1024, 2048, 512 -- see family_launch.hpp.
#define PAA_TRI_SHAPES_HERE(X) X(8, S1024) X(9, S2048) X(10, S512) X(11, S256)
#include <cstdlib>
#include <cstring>

#include "family_tri_launch.hpp"

namespace paa {
namespace launch {
int tri_part_c(const tri::TriLaunch &tl, const TileArgs &a) { return tri_here(tl, a); }
PAA_PHASE_READER(phase_tri_c)
}  // namespace launch
}  // namespace paa
