// The batched SMO solver and the one-against-one vote of the SVM split sweep (kernels_smo.hpp: the SVM fits of
// audioTrainTest.evaluate_classifier; kernels_smocache.hpp: the same solver over resident kernel matrices) and the sigmoid fit of probabilistic SVMs (kernels_platt.hpp) -- own translation unit,
// see model_launch.hpp.  The glue kernels of batched silence removal (kernels_onset.hpp) live here with the fit they surround.
#include "model_launch.hpp"
#include "kernels_smo.hpp"
#include "kernels_smocache.hpp"
#include "kernels_platt.hpp"
#include "kernels_onset.hpp"

namespace paa {
namespace launch {

int smo_step(const smo::SmoDev &m, const int *d_live, int n_live, int n_max, int budget, hipStream_t stream) {
    if (m.n_dims < 1 || m.n_dims > smo::kMaxDims || n_max < 1 || n_max > smo::kMaxRows) return -2;
    if (n_live < 1 || budget < 1) return -1;
    const int pitch = (m.n_dims + smo::kGroupLanes - 1) / smo::kGroupLanes * smo::kGroupLanes;
    const size_t lds = ((size_t)4 * pitch + n_max) * sizeof(double);
    if (raise_lds(reinterpret_cast<const void *>(&smo::smo_kernel), lds)) return -1;
    hipLaunchKernelGGL(smo::smo_kernel, dim3((unsigned)n_live), dim3(smo::kThreads), lds, stream, m, d_live, budget);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int smo_cached_step(const smo::SmoDev &m, const smo::SmoCacheDev &c, const int *d_live, int n_live, int budget, hipStream_t stream) {
    if (n_live < 1 || budget < 1) return -1;
    hipLaunchKernelGGL(smo::smo_cached_kernel, dim3((unsigned)n_live), dim3(smo::kThreads), 0, stream, m, c, d_live, budget);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int svc_pairs(const smo::SvcFitDev &f, long long n_blocks, int *d_label, double *d_dec, hipStream_t stream) {
    if (f.n_dims < 1 || f.n_dims > smo::kMaxDims || n_blocks < 1 || n_blocks > 0x7fffffffLL) return -1;
    const int pitch = (f.n_dims + smo::kGroupLanes - 1) / smo::kGroupLanes * smo::kGroupLanes;
    const size_t lds = ((size_t)smo::kTile * pitch + smo::kTile) * sizeof(double);
    if (raise_lds(reinterpret_cast<const void *>(&smo::svc_pairs_kernel), lds)) return -1;
    hipLaunchKernelGGL(smo::svc_pairs_kernel, dim3((unsigned)n_blocks), dim3(smo::kThreads), lds, stream, f, d_label, d_dec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int platt_sigmoid(const platt::PlattDev &p, int n_problems, int l_max, hipStream_t stream) {
    if (l_max < 1 || l_max > platt::kMaxRows) return -2;
    if (n_problems < 1) return -1;
    const size_t lds = ((size_t)l_max * 9 + 7) / 8 * 8;
    if (raise_lds(reinterpret_cast<const void *>(&platt::platt_sigmoid_kernel), lds)) return -1;
    hipLaunchKernelGGL(platt::platt_sigmoid_kernel, dim3((unsigned)n_problems), dim3(platt::kThreads), lds, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int onset_select(const onset::OnsetDev &m, int n_clips, hipStream_t stream) {
    if (n_clips < 1) return -1;
    hipLaunchKernelGGL(onset::onset_select_kernel, dim3((unsigned)n_clips), dim3(onset::kThreads), 0, stream, m);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int onset_gather(const onset::OnsetDev &m, int n_clips, hipStream_t stream) {
    if (n_clips < 1 || m.n_dims < 1 || m.n_dims > onset::kMaxDims) return -1;
    hipLaunchKernelGGL(onset::onset_gather_kernel, dim3((unsigned)n_clips), dim3(onset::kThreads), 0, stream, m);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int onset_weights(const onset::OnsetDev &m, int n_clips, hipStream_t stream) {
    if (n_clips < 1 || m.n_dims < 1 || m.n_dims > onset::kMaxDims) return -1;
    hipLaunchKernelGGL(onset::onset_weights_kernel, dim3((unsigned)n_clips), dim3(onset::kThreads), 0, stream, m);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int onset_proba(const onset::OnsetDev &m, int n_clips, long long n_frames, hipStream_t stream) {
    const long long blocks = (n_frames + onset::kThreads - 1) / onset::kThreads;
    if (n_clips < 1 || n_frames < 1 || blocks > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(onset::onset_proba_kernel, dim3((unsigned)blocks), dim3(onset::kThreads), 0, stream, m, n_clips, n_frames);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int onset_threshold(const onset::OnsetDev &m, int n_clips, hipStream_t stream) {
    if (n_clips < 1) return -1;
    hipLaunchKernelGGL(onset::onset_threshold_kernel, dim3((unsigned)n_clips), dim3(onset::kThreads), 0, stream, m);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

void smo_geometry(int out6[6]) {
    out6[0] = smo::kThreads;
    out6[1] = smo::kGroups;
    out6[2] = smo::kMaxRows;
    out6[3] = smo::kQueriesPerBlock;
    out6[4] = smo::kDefaultItersPerLaunch;
    out6[5] = smo::kMaxDims;
}

}  // namespace launch
}  // namespace paa
