// The SVR fits of audioTrainTest.evaluate_regression (audioTrainTest.py:774-855 with train_svm_regression :222-226) as a batch of
// epsilon-SVR dual problems: libsvm's solve_epsilon_svr over its Solver (svm.cpp: Solve, select_working_set, calculate_rho)
// without shrinking, FP64 throughout, one workgroup per TASK.
// A task is a list of n rows of the resident sample matrix X, the mean / scale of its job (rows are standardised on the load
// path, (x - mean) / scale with an IEEE division, as smo_kernel does), C, gamma, epsilon and the resident targets y.
//
// The dual has 2 n variables: variable v stands for row v mod n, with the sign +1 for v < n and -1 for v >= n, the linear term
// epsilon - y_t for v = t and epsilon + y_t for v = t + n, and Q_uv = sign_u sign_v K(row u, row v).  svr_smo_kernel is smo_kernel
// over the indices 0 .. 2 n - 1 -- the same selections (the greatest -y G over I_up, the greatest index on a tie; the second-order
// choice of j; TAU), the same clip cases in their order, the same calculate_rho -- but a kernel row is formed ONCE PER ROW: the
// group that owns row t forms K(row i, t), keeps it in LDS (n doubles) and judges both candidates t and t + n from it (eta is
// K_ii + K_tt - 2 K_it for either sign); in the j pass the one K(row j, t) updates G_t and G_{t+n}, which move by opposite amounts.
// alpha and G (2 n) and K_tt (n) live in device memory between launches; an iteration reads nothing but (alpha, G): the result is
// bit-identical for any budget, alone or in any batch.
// At a stop the workgroup writes rho, the gap, beta_t = alpha_t - alpha_{t+n}, the number of rows with beta != 0 and the task's
// training predictions G_t - epsilon + y_t - rho: G_t = sum_s beta_s K_ts + epsilon - y_t is the gradient the solver holds.
#pragma once
#include "kernels_smo_core.hpp"

namespace paa {
namespace svrfit {

using namespace smo;

__global__ __launch_bounds__(kThreads) void svr_smo_kernel(SvrDev m, const int *__restrict__ live, int budget) {
    extern __shared__ double lds[];                     // mean [pitch] | scale [pitch] | zi [pitch] | zj [pitch] | Ki [n_max]
    __shared__ double red_v[kWaves];
    __shared__ int red_i[kWaves];
    __shared__ double red_sum[kGroups], red_ub[kGroups], red_lb[kGroups];
    __shared__ int red_free[kGroups], red_sv[kGroups];
    __shared__ double s_rho;
    const int tid = threadIdx.x, lane = tid % kGroupLanes, group = tid / kGroupLanes;
    const int task = live[blockIdx.x];
    const SmoTask T = m.tasks[task];
    const int n = T.n, n_dims = m.n_dims;
    const int M = (n_dims + kGroupLanes - 1) / kGroupLanes, pitch = M * kGroupLanes;
    double *s_mean = lds, *s_scale = lds + pitch, *zi = lds + 2 * pitch, *zj = lds + 3 * pitch, *Ki = lds + 4 * pitch;
    const int *__restrict__ idx = m.idx + T.off;
    double *alpha = m.alpha + 2 * T.off, *G = m.G + 2 * T.off, *QD = m.QD + T.off;
    const bool rbf = m.rbf != 0;
    const double C = T.C, gamma = T.gamma, epsilon = m.epsilon[task];
    for (int d = tid; d < pitch; d += kThreads) {
        s_mean[d] = d < n_dims ? m.mean[(long long)T.stat * n_dims + d] : 0.0;
        s_scale[d] = d < n_dims ? m.scale[(long long)T.stat * n_dims + d] : 1.0;
    }
    __syncthreads();
    int iter = m.iter[task];
    if (m.status[task] == kFresh) {                     // alpha = 0, G = epsilon -+ y, K_tt once per task
        for (int t = group; t < n; t += kGroups) {
            const double *__restrict__ x = m.X + (long long)idx[t] * n_dims;
            double acc = 0.0;
            if (!rbf)
                for (int i = 0; i < M; ++i) {
                    const int d = lane + kGroupLanes * i;
                    const double z = d < n_dims ? (x[d] - s_mean[d]) / s_scale[d] : 0.0;
                    acc = fma(z, z, acc);
                }
            acc = kv::group_sum(acc);
            if (lane == 0) {
                const double yt = m.y[idx[t]];
                QD[t] = rbf ? 1.0 : acc;                // exp(-gamma * 0)
                alpha[t] = 0.0;
                alpha[t + n] = 0.0;
                G[t] = epsilon - yt;
                G[t + n] = epsilon + yt;
            }
        }
        iter = 0;
        __syncthreads();
    }

    int status = kRunning;
    double gmax = 0.0, gmax2 = 0.0;
    bool both = false;                                  // I_up and I_low are not empty: the gap is a number
    for (int done = 0;; ++done) {
        // 1. i: the greatest v = -y G over I_up (ties: the greatest index); Gmax2 over I_low.  Row t carries the variables t, t + n
        double bv = 0.0, b2 = 0.0;
        int bi = -1, b2i = -1;
        for (int t = group; t < n; t += kGroups) {
            const double ap = alpha[t], an = alpha[t + n], vp = -G[t], vn = G[t + n];
            if (ap < C) take_max(bv, bi, vp, t);
            if (an > 0.0) take_max(bv, bi, vn, t + n);
            if (ap > 0.0) take_max(b2, b2i, -vp, t);
            if (an < C) take_max(b2, b2i, -vn, t + n);
        }
        block_max(bv, bi, red_v, red_i, tid);
        block_max(b2, b2i, red_v, red_i, tid);
        gmax = bv;
        gmax2 = b2;
        const int i = bi;
        both = bi >= 0 && b2i >= 0;
        if (i < 0 || b2i < 0 || !(gmax + gmax2 >= m.eps)) { status = kConverged; break; }
        if (iter >= m.max_iter) { status = kNotConverged; break; }
        if (done >= budget) break;

        // 2. K(row i, t) once per row, and j: the least -b^2 / eta over I_low with b > 0 (ties: the greatest index)
        const int ri = i < n ? i : i - n;
        stage_point(zi, m.X, idx[ri], n_dims, s_mean, s_scale, pitch, tid);
        __syncthreads();
        const double qd_i = QD[ri];
        double jv = 0.0;
        int ji = -1;
        for (int t = group; t < n; t += kGroups) {
            const double k = kernel_value(m.X, idx[t], zi, s_mean, s_scale, n_dims, M, lane, rbf, gamma);
            if (lane == 0) Ki[t] = k;
            double eta = qd_i + QD[t] - 2.0 * k;
            if (!(eta > 0.0)) eta = kTau;
            const double bp = gmax + G[t], bn = gmax - G[t + n];
            if (alpha[t] > 0.0 && bp > 0.0) take_max(jv, ji, (bp * bp) / eta, t);
            if (alpha[t + n] < C && bn > 0.0) take_max(jv, ji, (bn * bn) / eta, t + n);
        }
        block_max(jv, ji, red_v, red_i, tid);           // (its barriers also publish Ki)
        const int j = ji;
        if (j < 0) { status = kConverged; break; }

        // 3. the two-variable update (every thread, from the same values), then G
        const int rj = j < n ? j : j - n;
        const double yi = i < n ? 1.0 : -1.0, yj = j < n ? 1.0 : -1.0, ai = alpha[i], aj = alpha[j];
        double eta = qd_i + QD[rj] - 2.0 * Ki[rj];
        if (!(eta > 0.0)) eta = kTau;
        double ni, nj;
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
        const double ci = yi * (ni - ai), cj = yj * (nj - aj);
        stage_point(zj, m.X, idx[rj], n_dims, s_mean, s_scale, pitch, tid);
        __syncthreads();                                // every thread has read alpha and G of i and j
        for (int t = group; t < n; t += kGroups) {
            const double k = kernel_value(m.X, idx[t], zj, s_mean, s_scale, n_dims, M, lane, rbf, gamma);
            if (lane == 0) {
                const double w = Ki[t] * ci + k * cj;   // Q_i,t d_alpha_i + Q_j,t d_alpha_j of the variable t; t + n moves by -w
                G[t] += w;
                G[t + n] -= w;
            }
        }
        if (tid == 0) { alpha[i] = ni; alpha[j] = nj; }
        ++iter;
        __syncthreads();                                // G and alpha of this iteration before the next scan
    }

    if (status == kRunning) {
        if (tid == 0) { m.iter[task] = iter; m.status[task] = kRunning; }
        return;
    }
    // rho (calculate_rho over the 2 n variables), beta and the support-vector count
    double sum = 0.0, ub = __builtin_inf(), lb = -__builtin_inf();
    int n_free = 0, n_sv = 0;
    for (int t = group; t < n; t += kGroups) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const double a = alpha[t + h * n], y = h ? -1.0 : 1.0, yG = y * G[t + h * n];
            if (a > 0.0 && a < C) { sum += yG; ++n_free; }
            else if ((a >= C) == (y < 0.0)) ub = fmin(ub, yG);
            else lb = fmax(lb, yG);
        }
        const double beta = alpha[t] - alpha[t + n];
        n_sv += beta != 0.0;
        if (lane == 0) m.beta[T.off + t] = beta;
    }
    if (lane == 0) { red_sum[group] = sum; red_ub[group] = ub; red_lb[group] = lb; red_free[group] = n_free; red_sv[group] = n_sv; }
    __syncthreads();
    if (tid == 0) {
        for (int g = 1; g < kGroups; ++g) {
            sum += red_sum[g];
            ub = fmin(ub, red_ub[g]);
            lb = fmax(lb, red_lb[g]);
            n_free += red_free[g];
            n_sv += red_sv[g];
        }
        const double rho = n_free > 0 ? sum / (double)n_free : (ub + lb) / 2.0;
        s_rho = rho;
        m.rho[task] = rho;
        m.gap[task] = both ? gmax + gmax2 : 0.0;
        m.n_sv[task] = n_sv;
        m.iter[task] = iter;
        m.status[task] = status;
    }
    __syncthreads();
    // the training predictions from the gradient: G_t = sum_s beta_s K_ts + epsilon - y_t
    const double rho = s_rho;
    for (int t = group; t < n; t += kGroups)
        if (lane == 0) m.train_pred[T.off + t] = G[t] - epsilon + m.y[idx[t]] - rho;
}

}  // namespace svrfit
}  // namespace paa
