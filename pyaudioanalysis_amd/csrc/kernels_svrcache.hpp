// The resident kernel matrix of the SVR solver (DESIGN K22): svr_smo_kernel (kernels_svrfit.hpp) forms K(row i, .) and K(row j, .)
// anew in every iteration; here the n x n matrix of a task is formed ONCE, by the whole device, and a second solver reads its rows.
//   svr_standardise_kernel   Z [n][pitch] of every task of a chunk: (x - mean) / scale with the IEEE division of stage_point and
//                            kernel_value, zero beyond n_dims (pitch = 8 ceil(n_dims / 8))
//   svr_gram_kernel          K [n][n] of every task of a chunk; the grid runs over (task, tile pair a <= b) of kGramTile rows.  Every
//                            value is the bits of smo::kernel_value: an 8-lane group owns a value, lane l runs the fma chain over
//                            the dims l, l + 8, ... in that order, kv::group_sum, then exp(-gamma acc) for RBF.  The chain is
//                            symmetric in its two rows (a product commutes, (a - b)^2 = (b - a)^2), so a tile pair is formed once and
//                            written twice, both times along rows, through an LDS tile.  No FP64 matrix core: it sums in another order
//   svr_smo_cached_kernel    the iteration of svr_smo_kernel on the same pieces of the solver core (kernels_smo_core.hpp: block_max,
//                            clamp_eta, pair_update, RhoPartial, suspend), with K_i[t], K_j[t] and K_tt read from the matrix and one
//                            THREAD per row in the scan, the j pass and the G update (the selections are exact: the greatest value,
//                            then the greatest index, whatever the order); calculate_rho's sum runs on RhoPartial's group mapping,
//                            the one place where another mapping would change bits.  Bit-identical to svr_smo_kernel in every output
// All offsets into Z and K are 64-bit.
#pragma once
#include "kernels_svrfit.hpp"

namespace paa {
namespace svrfit {

// one workgroup per (task of the chunk, kGramTile rows)
__global__ __launch_bounds__(kThreads) void svr_standardise_kernel(SvrDev m, SvrCacheDev c, const int *__restrict__ chunk) {
    const int task = chunk[blockIdx.x];
    const SmoTask T = m.tasks[task];
    const int n_dims = m.n_dims, pitch = (n_dims + kGroupLanes - 1) / kGroupLanes * kGroupLanes;
    const int r0 = blockIdx.y * kGramTile;
    if (r0 >= T.n) return;
    const int rows = min(kGramTile, T.n - r0);
    const int *__restrict__ idx = m.idx + T.off;
    const double *__restrict__ mean = m.mean + (long long)T.stat * n_dims;
    const double *__restrict__ scale = m.scale + (long long)T.stat * n_dims;
    double *__restrict__ Z = c.Z + c.z_off[task] + (long long)r0 * pitch;
    for (int e = threadIdx.x; e < rows * pitch; e += kThreads) {
        const int r = e / pitch, d = e % pitch;
        Z[e] = d < n_dims ? (m.X[(long long)idx[r0 + r] * n_dims + d] - mean[d]) / scale[d] : 0.0;
    }
}

// one workgroup per tile pair: rows a0 .. a0 + 31 (one per group, in registers) against rows b0 .. b0 + 31 (LDS)
__global__ __launch_bounds__(kThreads) void svr_gram_kernel(SvrDev m, SvrCacheDev c, const GramTile *__restrict__ tiles) {
    extern __shared__ double lds[];                     // zb [kGramTile][pitch] | out [kGramTile][kGramTile + 1]
    const int tid = threadIdx.x, lane = tid % kGroupLanes, group = tid / kGroupLanes;
    const GramTile W = tiles[blockIdx.x];
    const SmoTask T = m.tasks[W.task];
    const int n = T.n, n_dims = m.n_dims;
    const int M = (n_dims + kGroupLanes - 1) / kGroupLanes, pitch = M * kGroupLanes;
    const int a0 = W.a * kGramTile, b0 = W.b * kGramTile;
    const int na = min(kGramTile, n - a0), nb = min(kGramTile, n - b0);
    double *zb = lds, *out = lds + kGramTile * pitch;
    const double *__restrict__ Z = c.Z + c.z_off[W.task];
    double *__restrict__ K = c.K + c.k_off[W.task];
    const bool rbf = m.rbf != 0;
    const double gamma = T.gamma;
    for (int e = tid; e < nb * pitch; e += kThreads) zb[e] = Z[(long long)b0 * pitch + e];
    double x[kMaxM];
    const bool live = group < na;
#pragma unroll
    for (int i = 0; i < kMaxM; ++i) x[i] = (i < M && live) ? Z[(long long)(a0 + group) * pitch + lane + kGroupLanes * i] : 0.0;
    __syncthreads();
    for (int r = 0; r < nb; ++r) {
        const double *t = zb + r * pitch + lane;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < kMaxM; ++i) {
            if (i < M) {
                if (rbf) {
                    const double df = x[i] - t[kGroupLanes * i];
                    acc = fma(df, df, acc);
                } else {
                    acc = fma(x[i], t[kGroupLanes * i], acc);
                }
            }
        }
        acc = kv::group_sum(acc);
        if (lane == 0) out[group * (kGramTile + 1) + r] = rbf ? exp(-gamma * acc) : acc;
    }
    __syncthreads();
    for (int e = tid; e < kGramTile * kGramTile; e += kThreads) {
        const int r = e / kGramTile, q = e % kGramTile;
        if (r < na && q < nb) K[(long long)(a0 + r) * n + b0 + q] = out[r * (kGramTile + 1) + q];
        if (W.a != W.b && r < nb && q < na) K[(long long)(b0 + r) * n + a0 + q] = out[q * (kGramTile + 1) + r];
    }
}

// a body of its own beside svr_smo_kernel's: as two instances of one template over the rows' owner and source this one measured 0.7 %
// slower (3.113 / 3.119 s against 3.091 / 3.094 s for the capped linear sweep), with the same instructions in its loop
__global__ __launch_bounds__(kThreads) void svr_smo_cached_kernel(SvrDev m, SvrCacheDev c, const int *__restrict__ live, int budget) {
    const SolverLds s = solver_lds();
    const int tid = threadIdx.x, lane = tid % kGroupLanes, group = tid / kGroupLanes;
    const int task = live[blockIdx.x];
    const SmoTask T = m.tasks[task];
    const int n = T.n;
    const int *__restrict__ idx = m.idx + T.off;
    const double *__restrict__ K = c.K + c.k_off[task];
    double *alpha = m.alpha + 2 * T.off, *G = m.G + 2 * T.off, *QD = m.QD + T.off;
    const bool rbf = m.rbf != 0;
    const double C = T.C, epsilon = m.epsilon[task];
    int iter = m.iter[task];
    if (m.status[task] == kFresh) {                     // alpha = 0, G = epsilon -+ y, K_tt from the diagonal
        for (int t = tid; t < n; t += kThreads) {
            const double yt = m.y[idx[t]];
            QD[t] = rbf ? 1.0 : K[(long long)t * n + t];
            alpha[t] = 0.0;
            alpha[t + n] = 0.0;
            G[t] = epsilon - yt;
            G[t + n] = epsilon + yt;
        }
        iter = 0;
        __syncthreads();
    }

    int status = kRunning;
    double gmax = 0.0, gmax2 = 0.0;
    bool both = false;
    for (int done = 0;; ++done) {
        // 1. i and Gmax2
        double bv = 0.0, b2 = 0.0;
        int bi = -1, b2i = -1;
        for (int t = tid; t < n; t += kThreads) {
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

        // 2. j over the resident row K(row i, .)
        const int ri = i < n ? i : i - n;
        const double *__restrict__ Ki = K + (long long)ri * n;
        const double qd_i = QD[ri];
        double jv = 0.0;
        int ji = -1;
        for (int t = tid; t < n; t += kThreads) {
            const double k = Ki[t];
            const double eta = clamp_eta(qd_i, QD[t], k);
            const double bp = gmax + G[t], bn = gmax - G[t + n];
            if (alpha[t] > 0.0 && bp > 0.0) take_max(jv, ji, (bp * bp) / eta, t);
            if (alpha[t + n] < C && bn > 0.0) take_max(jv, ji, (bn * bn) / eta, t + n);
        }
        block_max(jv, ji, s, tid);
        const int j = ji;
        if (j < 0) { status = kConverged; break; }

        // 3. the two-variable update (every thread, from the same values), then G over the rows K(row i, .) and K(row j, .)
        const int rj = j < n ? j : j - n;
        const double yi = i < n ? 1.0 : -1.0, yj = j < n ? 1.0 : -1.0, ai = alpha[i], aj = alpha[j];
        double ni, nj;
        pair_update(yi, yj, ai, aj, G, i, j, clamp_eta(qd_i, QD[rj], Ki[rj]), C, ni, nj);
        const double ci = yi * (ni - ai), cj = yj * (nj - aj);
        const double *__restrict__ Kj = K + (long long)rj * n;
        __syncthreads();                                // every thread has read alpha and G of i and j
        for (int t = tid; t < n; t += kThreads) {
            const double k = Kj[t];
            const double w = Ki[t] * ci + k * cj;
            G[t] += w;
            G[t + n] -= w;
        }
        if (tid == 0) { alpha[i] = ni; alpha[j] = nj; }
        ++iter;
        __syncthreads();                                // G and alpha of this iteration before the next scan
    }

    if (status == kRunning) { suspend(m.iter, m.status, task, iter, tid); return; }
    // rho, beta and the support-vector count on the group mapping (the solver core's order of rho's sum), then the training predictions
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
    for (int t = tid; t < n; t += kThreads) m.train_pred[T.off + t] = G[t] - epsilon + m.y[idx[t]] - rho;
}

}  // namespace svrfit
}  // namespace paa
