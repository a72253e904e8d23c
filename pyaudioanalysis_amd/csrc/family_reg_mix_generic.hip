// The in-place mixed-radix kernel (kernels_mix.hpp) and the generic Stockham kernel (kernels_generic.hpp) -- own translation
// unit, see family_launch.hpp.  (The prime-factor kernel st_reg that gave the unit its name left the tree in round 6:
// scripts/experiments/kernels_reg.hpp.)
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "family_launch.hpp"

namespace paa {
namespace launch {

template <typename T, int TWG, int LEAN>
static int mix_one(const mix::MixLayout &ml, const TileArgs &a) {
    static LdsAttrCache attr;
    return tile_launch(&mix::st_mix_kernel<T, TWG, LEAN>, attr, ml.waves, mix::mix_lds_bytes(ml), ml, a);
}
template <typename T>
static int mix_any(const mix::MixLayout &ml, const TileArgs &a) {
    if (ml.lean && ml.pad_shift == 5) return ml.tw_global ? mix_one<T, 1, 2>(ml, a) : mix_one<T, 0, 2>(ml, a);
    if (ml.lean) return ml.tw_global ? mix_one<T, 1, 1>(ml, a) : mix_one<T, 0, 1>(ml, a);
    return ml.tw_global ? mix_one<T, 1, 0>(ml, a) : mix_one<T, 0, 0>(ml, a);
}
int mix(const mix::MixLayout &ml, const TileArgs &a) {
    return with_sample_type(a.sample_kind, [&](auto tag) { return mix_any<PAA_SAMPLE_T(tag)>(ml, a); });
}

template <typename T>
static int generic_one(const GenLayout &gl, const TileArgs &a) {
    static LdsAttrCache attr;
    return tile_launch(&st_generic_kernel<T>, attr, gl.waves, generic_lds_bytes(gl), gl, a);
}
int generic(const GenLayout &gl, const TileArgs &a) {
    return with_sample_type(a.sample_kind, [&](auto tag) { return generic_one<PAA_SAMPLE_T(tag)>(gl, a); });
}

PAA_PHASE_READER(phase_rmg)
}  // namespace launch
}  // namespace paa
