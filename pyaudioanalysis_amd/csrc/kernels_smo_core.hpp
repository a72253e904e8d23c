// What the SMO solvers share on the device (kernels_smo.hpp: smo_kernel, the C-SVC dual; kernels_svrfit.hpp: svr_smo_kernel, the
// epsilon-SVR dual): the workgroup's (greatest value, then greatest index) reduction behind both selections, the staging of a
// standardised point in LDS and the kernel value of a row of X against it, on the lane split of kernels_kv.hpp.
#pragma once
#include "kernels_kv.hpp"
#include "model_launch.hpp"

namespace paa {
namespace smo {

using kv::kGroupLanes;
using kv::kMaxM;
using kv::kTile;
static_assert(kMaxDims <= kv::kMaxDims && kThreads % 64 == 0 && kGroups * kGroupLanes == kThreads, "groups of 8 lanes");
constexpr int kWaves = kThreads / 64;
constexpr double kTau = 1e-12;

// (a, i) replaces (b, j) when a is greater, or equal with a greater index; an index < 0 is "none"
__device__ __forceinline__ void take_max(double &b, int &j, double a, int i) {
    if (i >= 0 && (j < 0 || a > b || (a == b && i > j))) { b = a; j = i; }
}
__device__ __forceinline__ void wave_max(double &v, int &i) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        take_max(v, i, ov, oi);
    }
}
// the workgroup's (greatest value, then greatest index); red_v / red_i [kWaves] in LDS.  Every thread returns the same pair
__device__ __forceinline__ void block_max(double &v, int &i, double *red_v, int *red_i, int tid) {
    wave_max(v, i);
    __syncthreads();                                    // the previous use of red_* is over
    if (tid % 64 == 0) { red_v[tid / 64] = v; red_i[tid / 64] = i; }
    __syncthreads();
    v = red_v[0];
    i = red_i[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) take_max(v, i, red_v[w], red_i[w]);
}

// zs [pitch] = row `s` of X standardised, zero beyond n_dims (the whole workgroup; the caller synchronises)
__device__ __forceinline__ void stage_point(double *zs, const double *X, int s, int n_dims, const double *mean, const double *scale,
                                            int pitch, int tid) {
    for (int d = tid; d < pitch; d += kThreads) zs[d] = d < n_dims ? (X[(long long)s * n_dims + d] - mean[d]) / scale[d] : 0.0;
}

// K(z_t, z) of row `s` of X against the staged point zs, for the calling group (every lane gets the value)
__device__ __forceinline__ double kernel_value(const double *__restrict__ X, int s, const double *zs, const double *mean,
                                               const double *scale, int n_dims, int M, int lane, bool rbf, double gamma) {
    const double *__restrict__ x = X + (long long)s * n_dims;
    double acc = 0.0;
    for (int i = 0; i < M; ++i) {
        const int d = lane + kGroupLanes * i;
        const double z = d < n_dims ? (x[d] - mean[d]) / scale[d] : 0.0;
        if (rbf) {
            const double df = z - zs[d];
            acc = fma(df, df, acc);
        } else {
            acc = fma(z, zs[d], acc);
        }
    }
    acc = kv::group_sum(acc);
    return rbf ? exp(-gamma * acc) : acc;
}

}  // namespace smo
}  // namespace paa
