// The SVR fits of audioTrainTest.evaluate_regression (audioTrainTest.py:774-855 with train_svm_regression :222-226) as a batch of
// epsilon-SVR dual problems: libsvm's solve_epsilon_svr over its Solver, on the solver core of kernels_smo_core.hpp, one workgroup
// per TASK.
// A task is a list of n rows of the resident sample matrix X, the mean / scale of its job (rows are standardised on the load
// path, (x - mean) / scale with an IEEE division, as smo_kernel does), C, gamma, epsilon and the resident targets y.
//
// The dual has 2 n variables: variable v stands for row v mod n, with the sign +1 for v < n and -1 for v >= n, the linear term
// epsilon - y_t for v = t and epsilon + y_t for v = t + n, and Q_uv = sign_u sign_v K(row u, row v).  svr_smo_kernel is smo_kernel's
// iteration over the indices 0 .. 2 n - 1 -- the same selections, the same update (pair_update), the same calculate_rho (RhoPartial)
// -- but a kernel row is formed ONCE PER ROW: the group that owns row t forms K(row i, t), keeps it in LDS (n doubles) and judges both
// candidates t and t + n from it (eta is K_ii + K_tt - 2 K_it for either sign); in the j pass the one K(row j, t) updates G_t and
// G_{t+n}, which move by opposite amounts.
// alpha and G (2 n) and K_tt (n) live in device memory between launches.
// At a stop the workgroup writes rho, the gap, beta_t = alpha_t - alpha_{t+n}, the number of rows with beta != 0 and the task's
// training predictions G_t - epsilon + y_t - rho: G_t = sum_s beta_s K_ts + epsilon - y_t is the gradient the solver holds.
// svr_smo_cached_kernel (kernels_svrcache.hpp) is the same iteration over a resident matrix, one thread per row.  The two are two
// bodies over the core's pieces: written once over a type for the rows' owner and source, the cached solver measured 0.7 % slower.
#pragma once
#include "kernels_smo_core.hpp"

namespace paa {
namespace svrfit {

using namespace smo;

__global__ __launch_bounds__(kThreads) void svr_smo_kernel(SvrDev m, const int *__restrict__ live, int budget) {
    extern __shared__ double lds[];
    const SolverLds s = solver_lds();
    const int tid = threadIdx.x, lane = tid % kGroupLanes, group = tid / kGroupLanes;
    const int task = live[blockIdx.x];
    const SmoTask T = m.tasks[task];
    const int n = T.n, n_dims = m.n_dims;
    const int M = (n_dims + kGroupLanes - 1) / kGroupLanes, pitch = M * kGroupLanes;
    const PointLds p(lds, pitch);
    const int *__restrict__ idx = m.idx + T.off;
    double *alpha = m.alpha + 2 * T.off, *G = m.G + 2 * T.off, *QD = m.QD + T.off;
    const bool rbf = m.rbf != 0;
    const double C = T.C, gamma = T.gamma, epsilon = m.epsilon[task];
    stage_stats(p.mean, p.scale, m.mean, m.scale, T.stat, n_dims, pitch, tid);
    __syncthreads();
    int iter = m.iter[task];
    if (m.status[task] == kFresh) {                     // alpha = 0, G = epsilon -+ y, K_tt once per task
        for (int t = group; t < n; t += kGroups) {
            const double qd = rbf ? 1.0 : self_kernel(m.X, idx[t], p.mean, p.scale, n_dims, M, lane);
            if (lane == 0) {
                const double yt = m.y[idx[t]];
                QD[t] = qd;
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
        block_max(bv, bi, s, tid);
        block_max(b2, b2i, s, tid);
        gmax = bv;
        gmax2 = b2;
        const int i = bi;
        both = bi >= 0 && b2i >= 0;
        if (i < 0 || b2i < 0 || !(gmax + gmax2 >= m.eps)) { status = kConverged; break; }
        if (iter >= m.max_iter) { status = kNotConverged; break; }
        if (done >= budget) break;

        // 2. K(row i, t) once per row, and j: the least -b^2 / eta over I_low with b > 0 (ties: the greatest index)
        const int ri = i < n ? i : i - n;
        stage_point(p.zi, m.X, idx[ri], n_dims, p.mean, p.scale, pitch, tid);
        __syncthreads();
        const double qd_i = QD[ri];
        double jv = 0.0;
        int ji = -1;
        for (int t = group; t < n; t += kGroups) {
            const double k = kernel_value(m.X, idx[t], p.zi, p.mean, p.scale, n_dims, M, lane, rbf, gamma);
            if (lane == 0) p.Ki[t] = k;
            const double eta = clamp_eta(qd_i, QD[t], k);
            const double bp = gmax + G[t], bn = gmax - G[t + n];
            if (alpha[t] > 0.0 && bp > 0.0) take_max(jv, ji, (bp * bp) / eta, t);
            if (alpha[t + n] < C && bn > 0.0) take_max(jv, ji, (bn * bn) / eta, t + n);
        }
        block_max(jv, ji, s, tid);                      // (its barriers also publish Ki)
        const int j = ji;
        if (j < 0) { status = kConverged; break; }

        // 3. the two-variable update (every thread, from the same values), then G
        const int rj = j < n ? j : j - n;
        const double yi = i < n ? 1.0 : -1.0, yj = j < n ? 1.0 : -1.0, ai = alpha[i], aj = alpha[j];
        double ni, nj;
        pair_update(yi, yj, ai, aj, G, i, j, clamp_eta(qd_i, QD[rj], p.Ki[rj]), C, ni, nj);
        const double ci = yi * (ni - ai), cj = yj * (nj - aj);
        stage_point(p.zj, m.X, idx[rj], n_dims, p.mean, p.scale, pitch, tid);
        __syncthreads();                                // every thread has read alpha and G of i and j
        for (int t = group; t < n; t += kGroups) {
            const double k = kernel_value(m.X, idx[t], p.zj, p.mean, p.scale, n_dims, M, lane, rbf, gamma);
            if (lane == 0) {
                const double w = p.Ki[t] * ci + k * cj;    // Q_i,t d_alpha_i + Q_j,t d_alpha_j of the variable t; t + n moves by -w
                G[t] += w;
                G[t + n] -= w;
            }
        }
        if (tid == 0) { alpha[i] = ni; alpha[j] = nj; }
        ++iter;
        __syncthreads();                                // G and alpha of this iteration before the next scan
    }

    if (status == kRunning) { suspend(m.iter, m.status, task, iter, tid); return; }
    // rho (calculate_rho over the 2 n variables), beta and the support-vector count
    RhoPartial r;
    for (int t = group; t < n; t += kGroups) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const double y = h ? -1.0 : 1.0;
            r.add(alpha[t + h * n], y, y * G[t + h * n], C);
        }
        const double beta = alpha[t] - alpha[t + n];
        r.n_sv += beta != 0.0;
        if (lane == 0) m.beta[T.off + t] = beta;
    }
    const double rho = r.finish<true>(m, task, both ? gmax + gmax2 : 0.0, iter, status, s, tid);
    // the training predictions from the gradient: G_t = sum_s beta_s K_ts + epsilon - y_t
    for (int t = group; t < n; t += kGroups)
        if (lane == 0) m.train_pred[T.off + t] = G[t] - epsilon + m.y[idx[t]] - rho;
}

}  // namespace svrfit
}  // namespace paa
