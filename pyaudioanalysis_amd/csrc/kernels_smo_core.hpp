// The solver core: what the SMO kernels share on the device (kernels_smo.hpp: smo_kernel, the C-SVC dual; kernels_svrfit.hpp:
// svr_smo_kernel and kernels_svrcache.hpp: svr_smo_cached_kernel, the epsilon-SVR dual).  All of it is libsvm's
// Solver (svm.cpp: Solve, select_working_set, calculate_rho) without shrinking, FP64 throughout, one workgroup per task:
//   selection    take_max / block_max: the workgroup's (greatest value, then greatest index) -- exact, associative and commutative,
//                so the order of the reduction cannot matter and no lane's timing does
//   a task       stage_stats (mean / scale in LDS), self_kernel (K_tt), stage_point and kernel_value (a standardised point in LDS
//                and the kernel value of a row of X against it, on the lane split of kernels_kv.hpp), clamp_eta (TAU)
//   the update   pair_update: the two branches of the two-variable step, each with its four clips IN THEIR ORDER
//   a stop       RhoPartial: calculate_rho, the support-vector count and the stores of a task's results.  The sum behind rho has
//                ONE association: a group adds its rows g, g + 32, ... in row order (both variables of an SVR row in the order t,
//                t + n), then thread 0 adds the groups 1 .. 31 to group 0's value in group order.  Every solver kernel, whatever
//                mapping its other passes use, runs this pass on the group mapping
//                suspend: the launch's budget ran out, the task goes on in the next launch
// alpha, G and K_tt live in device memory between launches; a launch runs at most `budget` iterations of a task and an iteration
// reads nothing but (alpha, G): the result is bit-identical for any budget, alone or in any batch.
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

// the static LDS of a solver kernel: block_max's pairs, the groups' partials of RhoPartial and rho for every thread.  The arrays are
// variables of their own, declared in solver_lds() alone, and a kernel holds their addresses: as members of one __shared__ struct they
// cost smo_kernel two VGPRs (66) and with them its eighth wave per SIMD
struct SolverLds {
    double *red_v;
    int *red_i;
    double *red_sum, *red_ub, *red_lb;
    int *red_free, *red_sv;
    double *s_rho;
};
__device__ __forceinline__ SolverLds solver_lds() {
    __shared__ double red_v[kWaves];
    __shared__ int red_i[kWaves];
    __shared__ double red_sum[kGroups], red_ub[kGroups], red_lb[kGroups];
    __shared__ int red_free[kGroups], red_sv[kGroups];
    __shared__ double s_rho;
    return {red_v, red_i, red_sum, red_ub, red_lb, red_free, red_sv, &s_rho};
}
// the dynamic LDS of a solver that forms its kernel rows: mean [pitch] | scale [pitch] | zi [pitch] | zj [pitch] | Ki [n_max]
struct PointLds {
    double *mean, *scale, *zi, *zj, *Ki;
    __device__ __forceinline__ PointLds(double *lds, int pitch)
        : mean(lds), scale(lds + pitch), zi(lds + 2 * pitch), zj(lds + 3 * pitch), Ki(lds + 4 * pitch) {}
};

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
// the workgroup's (greatest value, then greatest index).  Every thread returns the same pair
__device__ __forceinline__ void block_max(double &v, int &i, const SolverLds &s, int tid) {
    wave_max(v, i);
    __syncthreads();                                    // the previous use of red_* is over
    if (tid % 64 == 0) { s.red_v[tid / 64] = v; s.red_i[tid / 64] = i; }
    __syncthreads();
    v = s.red_v[0];
    i = s.red_i[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) take_max(v, i, s.red_v[w], s.red_i[w]);
}

// the budget ran out: the task's iteration count, and kRunning for the host's relaunch loop
__device__ __forceinline__ void suspend(int *iter_out, int *status_out, int task, int iter, int tid) {
    if (tid == 0) { iter_out[task] = iter; status_out[task] = kRunning; }
}

// s_mean / s_scale [pitch] = row `stat` of mean / scale, padded with 0 / 1 (the whole workgroup; the caller synchronises)
__device__ __forceinline__ void stage_stats(double *s_mean, double *s_scale, const double *mean, const double *scale, int stat, int n_dims,
                                            int pitch, int tid) {
    for (int d = tid; d < pitch; d += kThreads) {
        s_mean[d] = d < n_dims ? mean[(long long)stat * n_dims + d] : 0.0;
        s_scale[d] = d < n_dims ? scale[(long long)stat * n_dims + d] : 1.0;
    }
}

// zs [pitch] = row `s` of X standardised, zero beyond n_dims (the whole workgroup; the caller synchronises)
__device__ __forceinline__ void stage_point(double *zs, const double *X, int s, int n_dims, const double *mean, const double *scale,
                                            int pitch, int tid) {
    for (int d = tid; d < pitch; d += kThreads) zs[d] = d < n_dims ? (X[(long long)s * n_dims + d] - mean[d]) / scale[d] : 0.0;
}

// the linear K_tt of row `s` of X, for the calling group (every lane gets the value).  Under RBF K_tt is the literal 1.0: exp(-gamma * 0)
__device__ __forceinline__ double self_kernel(const double *__restrict__ X, int s, const double *mean, const double *scale, int n_dims,
                                              int M, int lane) {
    const double *__restrict__ x = X + (long long)s * n_dims;
    double acc = 0.0;
    for (int i = 0; i < M; ++i) {
        const int d = lane + kGroupLanes * i;
        const double z = d < n_dims ? (x[d] - mean[d]) / scale[d] : 0.0;
        acc = fma(z, z, acc);
    }
    return kv::group_sum(acc);
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

// eta of the pair (i, t) from K_ii, K_tt and K_it; libsvm's TAU where it is not positive
__device__ __forceinline__ double clamp_eta(double qd_i, double qd_t, double k) {
    double eta = qd_i + qd_t - 2.0 * k;
    if (!(eta > 0.0)) eta = kTau;
    return eta;
}

// The two-variable update of the pair (i, j) with the signs yi, yj, the values ai, aj and the gradient G: the new values ni, nj.  The
// order of the clips is libsvm's and part of the result.  G[i] and G[j] are read inside the branch that uses them
__device__ __forceinline__ void pair_update(double yi, double yj, double ai, double aj, const double *G, int i, int j, double eta,
                                            double C, double &ni, double &nj) {
    if (yi != yj) {
        const double delta = (-G[i] - G[j]) / eta, d = ai - aj;
        ni = ai + delta;
        nj = aj + delta;
        if (d > 0.0) { if (nj < 0.0) { nj = 0.0; ni = d; } }
        else { if (ni < 0.0) { ni = 0.0; nj = -d; } }
        if (d > 0.0) { if (ni > C) { ni = C; nj = C - d; } }
        else { if (nj > C) { nj = C; ni = C + d; } }
    } else {
        const double delta = (G[i] - G[j]) / eta, s = ai + aj;
        ni = ai - delta;
        nj = aj + delta;
        if (s > C) { if (ni > C) { ni = C; nj = s - C; } }
        else { if (nj < 0.0) { nj = 0.0; ni = s; } }
        if (s > C) { if (nj > C) { nj = C; ni = s - C; } }
        else { if (ni < 0.0) { ni = 0.0; nj = s; } }
    }
}

// calculate_rho and the support-vector count of a stopped task: a thread's partial over the variables of its group's rows
struct RhoPartial {
    double sum = 0.0, ub = __builtin_inf(), lb = -__builtin_inf();
    int n_free = 0, n_sv = 0;                           // n_sv: the caller counts

    // one variable: its value, its sign and y G
    __device__ __forceinline__ void add(double a, double y, double yG, double C) {
        if (a > 0.0 && a < C) { sum += yG; ++n_free; }
        else if ((a >= C) == (y < 0.0)) ub = fmin(ub, yG);          // {alpha = C, y = -1} and {alpha = 0, y = +1}
        else lb = fmax(lb, yG);
    }
    // thread 0 ends with the workgroup's values: the groups' partials in group order
    __device__ __forceinline__ void combine(const SolverLds &s, int tid) {
        const int lane = tid % kGroupLanes, group = tid / kGroupLanes;
        if (lane == 0) { s.red_sum[group] = sum; s.red_ub[group] = ub; s.red_lb[group] = lb; s.red_free[group] = n_free; s.red_sv[group] = n_sv; }
        __syncthreads();
        if (tid == 0) {
            for (int g = 1; g < kGroups; ++g) {
                sum += s.red_sum[g];
                ub = fmin(ub, s.red_ub[g]);
                lb = fmax(lb, s.red_lb[g]);
                n_free += s.red_free[g];
                n_sv += s.red_sv[g];
            }
        }
    }
    // combine, then the task's results (gap: Gmax + Gmax2, or 0 when I_up or I_low is empty).  kShare: every thread returns rho, at the
    // price of s_rho and one more barrier; without it the value returned means nothing
    template <bool kShare, class Dev>
    __device__ __forceinline__ double finish(const Dev &m, int task, double gap, int iter, int status, const SolverLds &s, int tid) {
        combine(s, tid);
        if (tid == 0) {
            const double rho = n_free > 0 ? sum / (double)n_free : (ub + lb) / 2.0;
            if (kShare) *s.s_rho = rho;
            m.rho[task] = rho;
            m.gap[task] = gap;
            m.n_sv[task] = n_sv;
            m.iter[task] = iter;
            m.status[task] = status;
        }
        if (!kShare) return 0.0;
        __syncthreads();
        return *s.s_rho;
    }
};

}  // namespace smo
}  // namespace paa
