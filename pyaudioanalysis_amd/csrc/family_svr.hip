// The bank of epsilon-SVR models (kernels_svr.hpp: audioTrainTest.regression_wrapper for the "svm" / "svm_rbf" models) --
// own translation unit, see model_launch.hpp.
#include <cstdlib>
#include <cstring>

#include "model_launch.hpp"
#include "kernels_svr.hpp"

namespace paa {
namespace launch {

int svr(const svr::SvrDev &m, const double *d_feats, long long ld, long long n_vec, double *d_out, long long ld_out,
        hipStream_t stream) {
    if (m.n_models < 1 || m.n_models > svr::kMaxModels || m.n_dims < 1 || m.n_dims > svr::kMaxDims || n_vec < 1 || ld < n_vec ||
        ld_out < n_vec)
        return -1;
    const long long xblocks = (n_vec + svr::kWinPerBlock - 1) / svr::kWinPerBlock;
    const int yblocks = (m.n_models + svr::kModelChunk - 1) / svr::kModelChunk;
    hipLaunchKernelGGL(svr::svr_bank_kernel, dim3((unsigned)xblocks, (unsigned)yblocks), dim3(svr::kThreads), 0, stream, m, d_feats,
                       ld, n_vec, d_out, ld_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

void svr_geometry(int out4[4]) {
    out4[0] = svr::kWinPerBlock;
    out4[1] = svr::kModelChunk;
    out4[2] = svr::kTile;
    out4[3] = svr::kGroupLanes;
}

}  // namespace launch
}  // namespace paa
