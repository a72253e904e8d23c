// The epsilon-SVR family: the bank of fitted models (kernels_svr.hpp: audioTrainTest.regression_wrapper for the "svm" / "svm_rbf"
// models) and the batched solver that fits them in the SVR split sweep (kernels_svrfit.hpp: the SVR fits of
// audioTrainTest.evaluate_regression; the sweep scores with svc_pairs_kernel of family_smo.hip) -- own translation unit, see
// model_launch.hpp.
#include <cstdlib>
#include <cstring>

#include "model_launch.hpp"
#include "kernels_svr.hpp"
#include "kernels_svrfit.hpp"
#include "kernels_svrcache.hpp"

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

int svr_smo_step(const svrfit::SvrDev &m, const int *d_live, int n_live, int n_max, int budget, hipStream_t stream) {
    if (m.n_dims < 1 || m.n_dims > smo::kMaxDims || n_max < 1 || n_max > smo::kMaxRows) return -2;
    if (n_live < 1 || budget < 1) return -1;
    const int pitch = (m.n_dims + smo::kGroupLanes - 1) / smo::kGroupLanes * smo::kGroupLanes;
    const size_t lds = ((size_t)4 * pitch + n_max) * sizeof(double);
    if (raise_lds(reinterpret_cast<const void *>(&svrfit::svr_smo_kernel), lds)) return -1;
    hipLaunchKernelGGL(svrfit::svr_smo_kernel, dim3((unsigned)n_live), dim3(smo::kThreads), lds, stream, m, d_live, budget);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int svr_gram(const svrfit::SvrDev &m, const svrfit::SvrCacheDev &c, const int *d_chunk, int n_chunk, int n_max,
             const svrfit::GramTile *d_tiles, long long n_tiles, hipStream_t stream) {
    static_assert(svrfit::kGramTile == smo::kGroups && svrfit::kPitchLanes == smo::kGroupLanes, "one row of a tile per group");
    if (m.n_dims < 1 || m.n_dims > smo::kMaxDims || n_max < 1 || n_max > svrfit::kGramMaxRows) return -2;
    if (n_chunk < 1 || n_tiles < 1 || n_tiles > 0x7fffffffLL) return -1;
    const int pitch = (m.n_dims + smo::kGroupLanes - 1) / smo::kGroupLanes * smo::kGroupLanes;
    const unsigned row_blocks = (unsigned)((n_max + svrfit::kGramTile - 1) / svrfit::kGramTile);
    hipLaunchKernelGGL(svrfit::svr_standardise_kernel, dim3((unsigned)n_chunk, row_blocks), dim3(smo::kThreads), 0, stream, m, c, d_chunk);
    if (hipGetLastError() != hipSuccess) return -1;
    const size_t lds = ((size_t)svrfit::kGramTile * pitch + svrfit::kGramTile * (svrfit::kGramTile + 1)) * sizeof(double);
    if (raise_lds(reinterpret_cast<const void *>(&svrfit::svr_gram_kernel), lds)) return -1;
    hipLaunchKernelGGL(svrfit::svr_gram_kernel, dim3((unsigned)n_tiles), dim3(smo::kThreads), lds, stream, m, c, d_tiles);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int svr_smo_cached_step(const svrfit::SvrDev &m, const svrfit::SvrCacheDev &c, const int *d_live, int n_live, int n_max, int budget,
                        hipStream_t stream) {
    if (n_max < 1 || n_max > smo::kMaxRows) return -2;
    if (n_live < 1 || budget < 1) return -1;
    hipLaunchKernelGGL(svrfit::svr_smo_cached_kernel, dim3((unsigned)n_live), dim3(smo::kThreads), 0, stream, m, c, d_live, budget);
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
