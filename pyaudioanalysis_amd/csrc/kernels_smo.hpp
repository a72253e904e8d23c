// The SVM fits of audioTrainTest.evaluate_classifier (audioTrainTest.py:631-700 with train_svm :132-155) as a batch of binary
// C-SVC dual problems: libsvm's Solver (svm.cpp: Solve, select_working_set, calculate_rho) without shrinking, FP64 throughout,
// one workgroup per TASK, and the one-against-one vote of svm_predict over the fitted tasks.
// A task is a list of rows of the resident sample matrix X, a sign per row, the mean / scale of its job (rows are
// standardised on the load path, (x - mean) / scale with an IEEE division, as in knn_split_kernel), C and gamma.
//
// smo_kernel, over the solver core of kernels_smo_core.hpp: the lane split of kernels_kv.hpp -- a group of 8 lanes owns the rows g,
// g + 32, g + 64, ... of the task and lane l the dims l, l + 8, ... of a row; three xor shuffles give every lane of the group the
// kernel value, so all eight lanes carry the same scalars and lane 0 stores.  Per iteration:
//   1. every group scans its rows for max v over I_up (v = -y G) and max -v over I_low; the workgroup reduces (block_max);
//   2. z_i is staged in LDS, every group forms K_it for its rows (kept in LDS: the gradient update needs it again), and in
//      the same pass the second-order objective -b^2 / eta of its rows; the workgroup reduces to j (least value, then
//      greatest index);
//   3. every thread computes the two-variable update from the same values (pair_update), z_j is staged, every group forms K_jt
//      and updates G_t of its rows.
// At a stop (converged or max_iter) the workgroup writes rho, the gap, alpha_t y_t and the number of support vectors (RhoPartial).
//
// svc_pairs_kernel: one group per test row of a job (32 rows per workgroup); per pair of the job the task's rows go through
// LDS tiles, standardised once per tile, and the rows with alpha != 0 add alpha_t y_t K(z_t, z) in train-list order.
#pragma once
#include "kernels_smo_core.hpp"

namespace paa {
namespace smo {

constexpr int kClassSlots = kMaxClasses / kGroupLanes;

__global__ __launch_bounds__(kThreads) void smo_kernel(SmoDev m, const int *__restrict__ live, int budget) {
    extern __shared__ double lds[];
    const SolverLds s = solver_lds();
    const int tid = threadIdx.x, lane = tid % kGroupLanes, group = tid / kGroupLanes;
    const int task = live[blockIdx.x];
    const SmoTask T = m.tasks[task];
    const int n = T.n, n_dims = m.n_dims;
    const int M = (n_dims + kGroupLanes - 1) / kGroupLanes, pitch = M * kGroupLanes;
    const PointLds p(lds, pitch);
    const int *__restrict__ idx = m.idx + T.off;
    const signed char *__restrict__ sign = m.sign + T.off;
    double *alpha = m.alpha + T.off, *G = m.G + T.off, *QD = m.QD + T.off;
    const bool rbf = m.rbf != 0;
    const double C = T.C, gamma = T.gamma;
    stage_stats(p.mean, p.scale, m.mean, m.scale, T.stat, n_dims, pitch, tid);
    __syncthreads();
    int iter = m.iter[task];
    if (m.status[task] == kFresh) {                     // alpha = 0, G = -1, K_tt once per task
        for (int t = group; t < n; t += kGroups) {
            const double qd = rbf ? 1.0 : self_kernel(m.X, idx[t], p.mean, p.scale, n_dims, M, lane);
            if (lane == 0) {
                QD[t] = qd;
                alpha[t] = 0.0;
                G[t] = -1.0;
            }
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
        for (int t = group; t < n; t += kGroups) {
            const double a = alpha[t], v = sign[t] > 0 ? -G[t] : G[t];
            const bool pos = sign[t] > 0;
            if (pos ? a < C : a > 0.0) take_max(bv, bi, v, t);
            if (pos ? a > 0.0 : a < C) take_max(b2, b2i, -v, t);
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

        // 2. K_it for every row, and j: the least -b^2 / eta over I_low with b > 0 (ties: the greatest index)
        stage_point(p.zi, m.X, idx[i], n_dims, p.mean, p.scale, pitch, tid);
        __syncthreads();
        const double qd_i = QD[i];
        double jv = 0.0;
        int ji = -1;
        for (int t = group; t < n; t += kGroups) {
            const double k = kernel_value(m.X, idx[t], p.zi, p.mean, p.scale, n_dims, M, lane, rbf, gamma);
            if (lane == 0) p.Ki[t] = k;
            const double a = alpha[t], v = sign[t] > 0 ? -G[t] : G[t];
            const bool pos = sign[t] > 0;
            const double b = gmax - v;
            // the greatest b^2 / eta is the least -b^2 / eta
            if ((pos ? a > 0.0 : a < C) && b > 0.0) take_max(jv, ji, (b * b) / clamp_eta(qd_i, QD[t], k), t);
        }
        block_max(jv, ji, s, tid);                      // (its barriers also publish Ki)
        const int j = ji;
        if (j < 0) { status = kConverged; break; }

        // 3. the two-variable update (every thread, from the same values), then G
        const double yi = sign[i], yj = sign[j], ai = alpha[i], aj = alpha[j];
        double ni, nj;
        pair_update(yi, yj, ai, aj, G, i, j, clamp_eta(qd_i, QD[j], p.Ki[j]), C, ni, nj);
        const double ci = yi * (ni - ai), cj = yj * (nj - aj);
        stage_point(p.zj, m.X, idx[j], n_dims, p.mean, p.scale, pitch, tid);
        __syncthreads();                                // every thread has read alpha and G of i and j
        for (int t = group; t < n; t += kGroups) {
            const double k = kernel_value(m.X, idx[t], p.zj, p.mean, p.scale, n_dims, M, lane, rbf, gamma);
            if (lane == 0) G[t] += (double)sign[t] * (p.Ki[t] * ci + k * cj);
        }
        if (tid == 0) { alpha[i] = ni; alpha[j] = nj; }
        ++iter;
        __syncthreads();                                // G and alpha of this iteration before the next scan
    }

    if (status == kRunning) { suspend(m.iter, m.status, task, iter, tid); return; }
    // rho (calculate_rho), alpha_t y_t and the support-vector count
    RhoPartial r;
    for (int t = group; t < n; t += kGroups) {
        const double a = alpha[t], y = sign[t];
        r.add(a, y, y * G[t], C);
        r.n_sv += a != 0.0;
        if (lane == 0) m.alpha_y[T.off + t] = a * y;
    }
    r.finish<false>(m, task, both ? gmax + gmax2 : 0.0, iter, status, s, tid);
}

// The one-against-one vote over the fitted tasks of a sweep (svm_predict, svm.cpp): workgroup b serves the test rows
// blocks[b].first .. + 31 of job blocks[b].job, one per group.  Per pair p = (a, b), a < b over the job's k present classes,
// dec = sum over the task's rows with alpha != 0, in the task's row order, of alpha_t y_t K(z_t, z) - rho; dec > 0 votes for a,
// otherwise b; the label is the first class with the most votes (its position among the job's classes).  dec_out
// [Q][max_pairs] may be null.
__global__ __launch_bounds__(kThreads) void svc_pairs_kernel(SvcFitDev f, int *__restrict__ label, double *__restrict__ dec_out) {
    extern __shared__ double lds[];                     // tile [kTile][pitch] | ay [kTile]
    const int tid = threadIdx.x, lane = tid % kGroupLanes, group = tid / kGroupLanes;
    const int n_dims = f.n_dims, M = (n_dims + kGroupLanes - 1) / kGroupLanes, pitch = M * kGroupLanes;
    double *tile = lds, *ay = lds + kTile * pitch;
    const knn::SplitBlock blk = f.blocks[blockIdx.x];
    const long long q0 = f.test_off[blk.job];
    const int n_test = (int)(f.test_off[blk.job + 1] - q0), k = f.job_k[blk.job], task0 = f.job_task[blk.job];
    const int stat = f.job_stat ? f.job_stat[blk.job] : blk.job;
    const double *__restrict__ mean = f.mean + (long long)stat * n_dims;
    const double *__restrict__ scale = f.scale + (long long)stat * n_dims;
    const int qi = blk.first + group;
    const bool live = qi < n_test;
    const long long q = q0 + qi;
    const double *__restrict__ xrow = f.X + (long long)(live ? f.test_idx[q] : 0) * n_dims;
    const bool rbf = f.rbf != 0;
    double x[kMaxM];
#pragma unroll
    for (int i = 0; i < kMaxM; ++i) {
        const int d = lane + kGroupLanes * i;
        x[i] = (i < M && d < n_dims && live) ? (xrow[d] - mean[d]) / scale[d] : 0.0;
    }
    int votes[kClassSlots];
#pragma unroll
    for (int s = 0; s < kClassSlots; ++s) votes[s] = 0;
    int p = 0;
    for (int a = 0; a < k; ++a) {
        for (int b = a + 1; b < k; ++b, ++p) {
            const SmoTask T = f.tasks[task0 + p];
            const int *__restrict__ idx = f.idx + T.off;
            const double *__restrict__ alpha_y = f.alpha_y + T.off;
            double dec = 0.0;
            for (int base = 0; base < T.n; base += kTile) {
                __syncthreads();
                for (int e = tid; e < kTile * pitch; e += kThreads) {
                    const int s = base + e / pitch, d = e % pitch;
                    tile[e] = (s < T.n && d < n_dims) ? (f.X[(long long)idx[s] * n_dims + d] - mean[d]) / scale[d] : 0.0;
                }
                if (tid < kTile) ay[tid] = base + tid < T.n ? alpha_y[base + tid] : 0.0;
                __syncthreads();
                for (int r = 0; r < kTile; ++r) {
                    const double c = ay[r];
                    if (c == 0.0) continue;             // not a support vector (the same for the whole workgroup)
                    const double *t = tile + r * pitch + lane;
                    double acc = 0.0;
#pragma unroll
                    for (int i = 0; i < kMaxM; ++i) {
                        if (i < M) {
                            if (rbf) {
                                const double df = t[kGroupLanes * i] - x[i];
                                acc = fma(df, df, acc);
                            } else {
                                acc = fma(t[kGroupLanes * i], x[i], acc);
                            }
                        }
                    }
                    acc = kv::group_sum(acc);
                    dec = fma(c, rbf ? exp(-T.gamma * acc) : acc, dec);
                }
            }
            dec -= f.rho[task0 + p];
            const int w = dec > 0.0 ? a : b;
#pragma unroll
            for (int s = 0; s < kClassSlots; ++s) votes[s] += w == lane + kGroupLanes * s;
            if (dec_out && live && lane == 0) dec_out[q * f.max_pairs + p] = dec;
        }
    }
    int key = -1;                                       // votes * 128 + (127 - class): the most votes, then the lowest class
#pragma unroll
    for (int s = 0; s < kClassSlots; ++s) {
        const int c = lane + kGroupLanes * s;
        if (c < k) key = max(key, votes[s] * 128 + (127 - c));
    }
#pragma unroll
    for (int o = 1; o < kGroupLanes; o <<= 1) key = max(key, __shfl_xor(key, o, kGroupLanes));
    if (live && lane == 0) label[q] = 127 - key % 128;
}

}  // namespace smo
}  // namespace paa
