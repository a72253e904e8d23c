// The real-input split of the long even windows on three register passes per sub-transform (kernels_wgs.hpp: 12 / 6 x 3675 samples = 44 100 /
// 22 050, 12 / 8 / 6 x 4000 = 48 000 / 32 000 / 24 000) -- own translation unit, see family_launch.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "family_launch.hpp"
#include "kernels_wgs.hpp"

namespace paa {
namespace launch {

// the family's shapes: f(WgsShape<R0, SH>()) of r0 x q samples, -1 for any other
template <int R0_, typename SH_> struct WgsShape {
    static constexpr int R0 = R0_;
    typedef SH_ SH;
};
template <typename F>
static int with_wgs_shape(int r0, int q, F &&f) {
    if (q == wgs::S3675::Q) {
        if (r0 == 12) return f(WgsShape<12, wgs::S3675>());
        if (r0 == 6) return f(WgsShape<6, wgs::S3675>());
    } else if (q == wgs::S4000::Q) {
        if (r0 == 12) return f(WgsShape<12, wgs::S4000>());
        if (r0 == 8) return f(WgsShape<8, wgs::S4000>());
        if (r0 == 6) return f(WgsShape<6, wgs::S4000>());
    }
    return -1;
}

template <typename T, int R0, typename SH>
static int wgs_one(const wg::FrameRef *tasks, int n_tasks, int *counter, const WgScratch &s, const WgArgs &a) {
    static LdsAttrCache attr;
    // one workgroup per CU; a multiple of eight (one segment of the task list per XCD) whenever every workgroup of such a grid has a task
    unsigned grid = (unsigned)std::min(n_tasks, a.num_cu);
    if (grid >= 64) grid &= ~7u;
    if (grid == 0) return 0;
    return wg_launch(&wgs::wgs_kernel<T, R0, SH>, attr, grid, SH::NT, (size_t)SH::LDS_BYTES, a.stream, a.P, (const T *)a.d_packed, a.clips, a.norms,
                     tasks, n_tasks, counter, s.spec, s.tfeat, s.psum, a.d_out);
}
int wgs(int r0, int q, const wg::FrameRef *tasks, int n_tasks, int *counter, const WgScratch &s, const WgArgs &a) {
    return with_wgs_shape(r0, q, [&](auto shape) {
        typedef decltype(shape) S;
        return with_sample_type(a.sample_kind, [&](auto tag) {
            return wgs_one<PAA_SAMPLE_T(tag), S::R0, typename S::SH>(tasks, n_tasks, counter, s, a);
        });
    });
}

template <int R0, int Q>
static int wgs_feat_one(const wg::FrameRef *frames, int n_frames, const WgScratch &s, const WgArgs &a) {
    static LdsAttrCache attr;
    if (n_frames <= 0) return 0;
    return wg_launch(&wgs::wgs_feat_kernel<R0, Q>, attr, 8u * (unsigned)((n_frames + 7) / 8), wgs::kFeatT, (size_t)wgs::feat_lds<R0, Q>(), a.stream,
                     a.P, frames, a.clips, n_frames, s.spec, s.tfeat, s.psum, a.d_out);
}
int wgs_feat(int r0, int q, const wg::FrameRef *frames, int n_frames, const WgScratch &s, const WgArgs &a) {
    return with_wgs_shape(r0, q, [&](auto shape) {
        typedef decltype(shape) S;
        return wgs_feat_one<S::R0, S::SH::Q>(frames, n_frames, s, a);
    });
}

}  // namespace launch
}  // namespace paa
