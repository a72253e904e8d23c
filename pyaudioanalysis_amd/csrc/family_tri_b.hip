// Three-pass register FFT (kernels_tri.hpp), second unit: 1764, 1920, 1600, 1200 and the two-pass 551 -- see family_launch.hpp.
#define PAA_TRI_SHAPES_HERE(X) X(2, S1764) X(3, S1920) X(4, S1600) X(5, S1200) X(6, S551)
#include <cstdlib>
#include <cstring>

#include "family_tri_launch.hpp"

namespace paa {
namespace launch {
int tri_part_b(const tri::TriLaunch &tl, const TileArgs &a) { return tri_here(tl, a); }
PAA_PHASE_READER(phase_tri_b)
}  // namespace launch
}  // namespace paa
