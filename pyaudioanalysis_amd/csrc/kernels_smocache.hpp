// The resident kernel matrix of the C-SVC solver (DESIGN K23): smo_kernel (kernels_smo.hpp) forms K(row i, .) and K(row j, .) anew in
// every iteration; here the tasks that standardise with the same mean / scale and use the same gamma -- a GROUP: the pair fits and the
// fold fits of one job -- share ONE matrix K [N][N] over the group's distinct rows, formed once by svr_standardise_kernel and
// svr_gram_kernel (kernels_svrcache.hpp: every value the bits of smo::kernel_value), and a second solver reads it.
//   smo_cached_kernel    the iteration of smo_kernel on the same pieces of the solver core (kernels_smo_core.hpp: block_max, clamp_eta,
//                        pair_update, RhoPartial, suspend).  Row t of a task is row pos[t] of its group's matrix: K_i[t] is
//                        K[pos[i] N + pos[t]], the linear K_tt the diagonal, 1.0 for RBF.  One THREAD per row in the scan, the j pass
//                        and the G update (the selections are exact: the greatest value, then the greatest index, whatever the
//                        order); calculate_rho's sum runs on RhoPartial's group mapping, the one place where another mapping would
//                        change bits.  No per-row LDS: nothing here bounds the rows of a task.  Bit-identical to smo_kernel in every
//                        output
// A pair task of a class-sorted group reads two contiguous runs of a matrix row (coalesced); a fold task reads a permuted subset of
// them (gathered, from L2 after the row's first touch).  All offsets into K are 64-bit.
#pragma once
#include "kernels_smo_core.hpp"

namespace paa {
namespace smo {

__global__ __launch_bounds__(kThreads) void smo_cached_kernel(SmoDev m, SmoCacheDev c, const int *__restrict__ live, int budget) {
    const SolverLds s = solver_lds();
    const int tid = threadIdx.x, lane = tid % kGroupLanes, group = tid / kGroupLanes;
    const int task = live[blockIdx.x];
    const SmoTask T = m.tasks[task];
    const int n = T.n;
    const long long N = c.group_n[task];
    const int *__restrict__ pos = c.pos + T.off;
    const signed char *__restrict__ sign = m.sign + T.off;
    const double *__restrict__ K = c.K + c.k_off[task];
    double *alpha = m.alpha + T.off, *G = m.G + T.off, *QD = m.QD + T.off;
    const bool rbf = m.rbf != 0;
    const double C = T.C;
    int iter = m.iter[task];
    if (m.status[task] == kFresh) {                     // alpha = 0, G = -1, K_tt from the diagonal
        for (int t = tid; t < n; t += kThreads) {
            QD[t] = rbf ? 1.0 : K[pos[t] * N + pos[t]];
            alpha[t] = 0.0;
            G[t] = -1.0;
        }
        iter = 0;
        __syncthreads();
    }

    int status = kRunning;
    double gmax = 0.0, gmax2 = 0.0;
    bool both = false;                                  // I_up and I_low are not empty: the gap is a number
    for (int done = 0;; ++done) {
        // 1. i: the greatest v over I_up (ties: the greatest index); Gmax2 over I_low
        double bv = 0.0, b2 = 0.0;
        int bi = -1, b2i = -1;
        for (int t = tid; t < n; t += kThreads) {
            const double a = alpha[t], v = sign[t] > 0 ? -G[t] : G[t];
            const bool pos_t = sign[t] > 0;
            if (pos_t ? a < C : a > 0.0) take_max(bv, bi, v, t);
            if (pos_t ? a > 0.0 : a < C) take_max(b2, b2i, -v, t);
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

        // 2. j over the resident row K(row i, .): the least -b^2 / eta over I_low with b > 0 (ties: the greatest index)
        const double *__restrict__ Ki = K + pos[i] * N;
        const double qd_i = QD[i];
        double jv = 0.0;
        int ji = -1;
        for (int t = tid; t < n; t += kThreads) {
            const double k = Ki[pos[t]];
            const double a = alpha[t], v = sign[t] > 0 ? -G[t] : G[t];
            const bool pos_t = sign[t] > 0;
            const double b = gmax - v;
            if ((pos_t ? a > 0.0 : a < C) && b > 0.0) take_max(jv, ji, (b * b) / clamp_eta(qd_i, QD[t], k), t);
        }
        block_max(jv, ji, s, tid);
        const int j = ji;
        if (j < 0) { status = kConverged; break; }

        // 3. the two-variable update (every thread, from the same values), then G over the rows K(row i, .) and K(row j, .)
        const double yi = sign[i], yj = sign[j], ai = alpha[i], aj = alpha[j];
        double ni, nj;
        pair_update(yi, yj, ai, aj, G, i, j, clamp_eta(qd_i, QD[j], Ki[pos[j]]), C, ni, nj);
        const double ci = yi * (ni - ai), cj = yj * (nj - aj);
        const double *__restrict__ Kj = K + pos[j] * N;
        __syncthreads();                                // every thread has read alpha and G of i and j
        for (int t = tid; t < n; t += kThreads) {
            const int p = pos[t];
            const double k = Kj[p];
            G[t] += (double)sign[t] * (Ki[p] * ci + k * cj);
        }
        if (tid == 0) { alpha[i] = ni; alpha[j] = nj; }
        ++iter;
        __syncthreads();                                // G and alpha of this iteration before the next scan
    }

    if (status == kRunning) { suspend(m.iter, m.status, task, iter, tid); return; }
    // rho (calculate_rho) on the group mapping (the solver core's order of rho's sum), alpha_t y_t and the support-vector count
    RhoPartial r;
    for (int t = group; t < n; t += kGroups) {
        const double a = alpha[t], y = sign[t];
        r.add(a, y, y * G[t], C);
        r.n_sv += a != 0.0;
        if (lane == 0) m.alpha_y[T.off + t] = a * y;
    }
    r.finish<false>(m, task, both ? gmax + gmax2 : 0.0, iter, status, s, tid);
}

}  // namespace smo
}  // namespace paa
