// The Bluestein (chirp-z) kernel (kernels_blu.hpp: windows whose FFT length has a prime factor above 13) -- own translation unit,
// see family_launch.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "family_launch.hpp"

namespace paa {
namespace launch {

template <typename T, int LOG2M, bool PK = false>
static int blu_one(const blu::BluLayout &bl, const TileArgs &a) {
    static LdsAttrCache attr;
    return tile_launch(&blu::st_blu_kernel<T, LOG2M, PK>, attr, bl.waves, blu::blu_lds_bytes(bl), bl, a);
}
template <typename T>
static int blu_any(const blu::BluLayout &bl, const TileArgs &a) {
    if (bl.packed) {
        switch (bl.log2m) {
            case 9: return blu_one<T, 9, true>(bl, a);
            case 10: return blu_one<T, 10, true>(bl, a);
            case 11: return blu_one<T, 11, true>(bl, a);
            case 12: return blu_one<T, 12, true>(bl, a);
            default: return -1;
        }
    }
    switch (bl.log2m) {
        case 8: return blu_one<T, 8>(bl, a);
        case 9: return blu_one<T, 9>(bl, a);
        case 10: return blu_one<T, 10>(bl, a);
        case 11: return blu_one<T, 11>(bl, a);
        case 12: return blu_one<T, 12>(bl, a);
        case 13: return blu_one<T, 13>(bl, a);
        default: return -1;
    }
}
int blu(const blu::BluLayout &bl, const TileArgs &a) {
    return with_sample_type(a.sample_kind, [&](auto tag) { return blu_any<PAA_SAMPLE_T(tag)>(bl, a); });
}

PAA_PHASE_READER(phase_blu)
}  // namespace launch
}  // namespace paa
