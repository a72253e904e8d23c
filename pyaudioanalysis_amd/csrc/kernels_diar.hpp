// Speaker diarization (audioSegmentation.speaker_diarization, :815-1056, lda_dim = 0): the clustering between the mid-term
// matrix and the HMM smoothing.  All FP64; every matrix is feature-major [n_dims][ld], window t in column t.
//
//  * standardize_kernel: scikit-learn's StandardScaler over the windows -- workgroup per feature row: mean, the corrected
//    two-pass population variance, scale = sqrt(var) or 1 for a constant row (scikit-learn's _is_constant_feature bound), and
//    Z = (x - mean) / scale.
//  * select_rows_kernel: Zk = the kept rows of Z.
//  * dimdist_kernel / dimdist_reduce_kernel: the reference's pdist(X.T): Euclidean distances between FEATURE ROWS over the
//    windows of a label subset (none: all windows); (k index, cluster) pairs of a sweep in one launch.  Thread (i, j) of a
//    16 x 16 tile walks the windows serially; then the column sums and the mean over the i < j pairs.
//  * k-means (Lloyd as scikit-learn 1.7 runs it, one initialisation): assign_kernel -- one lane per window, the squared
//    distances to all centres in the difference form sum_d (z_d - c_d)^2, centres staged in LDS by blocks of dims, lowest
//    index among equal minima; update_kernel -- workgroup per (feature row, k index): per-cluster sums, per-thread partials
//    in a fixed order and a fixed tree, no floating-point atomics; finish_kernel -- empty clusters moved to the windows
//    farthest from their centres, new centres, summed squared shift, and the convergence decision (labels unchanged, or
//    shift <= tol, or max_iter) left in a small per-k record the host polls.
//  * sqdist_points_kernel / get_points_kernel: k-means++ seeding's distance work (squared distances of all windows to a few
//    candidate windows) and the gather of chosen windows.
//  * pair_kernel: S[c][c2] = sum over windows i in c, j in c2 of |z_i - z_j| for every k of the sweep in ONE pass over the
//    window pairs (a pair's distance does not depend on k, only its bin does).  Workgroup per 128 x 128 tile on or above the
//    diagonal, panels of 8 dims in LDS, an 8 x 8 micro-tile of squared distances per thread (difference form: repeated
//    windows give exactly 0, the Gram expansion would cancel); then per k: row sums per column cluster (select + 16-lane
//    shuffle tree), binned by row cluster by one thread per (c, c2) walking the 128 rows in order.  Off-diagonal tiles
//    store P[c][c2] + P[c2][c].  pair_reduce_kernel adds the tiles' partials in tile order (two stages).
#pragma once
#include "device_common.hpp"
#include "model_launch.hpp"

namespace paa {
namespace diar {

constexpr int kThreads = 256;
constexpr int kDimChunk = 32;         // dims of the centres staged per step of assign_kernel
constexpr int kDimTile = 16;          // dimdist_kernel: feature rows per tile side
constexpr int kDimWin = 64;           // ... and windows staged per step
constexpr int kPairTile = 128;        // pair_kernel: windows per tile side
constexpr int kPairDims = 8;          // ... and dims per LDS panel (two panels + the row-sum table stay under 64 KB)

// sum over the workgroup in a fixed tree; `red` holds kThreads doubles
__device__ __forceinline__ double block_sum(double v, double *red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

// stats [3][n_dims]: mean, variance, scale
__global__ __launch_bounds__(kThreads) void standardize_kernel(const double *__restrict__ M, long long ldm, long long n, int n_dims,
                                                               double *__restrict__ Z, long long ldz, double *__restrict__ stats) {
    __shared__ double red[kThreads];
    const int d = blockIdx.x;
    const double *x = M + (long long)d * ldm;
    double s = 0.0;
    for (long long t = threadIdx.x; t < n; t += kThreads) s += x[t];
    const double mean = block_sum(s, red) / (double)n;
    double c = 0.0, ss = 0.0;
    for (long long t = threadIdx.x; t < n; t += kThreads) {
        const double df = x[t] - mean;
        c += df;
        ss = fma(df, df, ss);
    }
    c = block_sum(c, red);
    ss = block_sum(ss, red);
    double var = (ss - c * c / (double)n) / (double)n;
    const double eps = 2.220446049250313e-16;
    const double nm = (double)n * mean * eps;
    const bool constant = var <= (double)n * eps * var + nm * nm;
    const double scale = constant ? 1.0 : sqrt(var);
    for (long long t = threadIdx.x; t < n; t += kThreads) Z[(long long)d * ldz + t] = (x[t] - mean) / scale;
    if (threadIdx.x == 0) {
        stats[d] = mean;
        stats[n_dims + d] = var;
        stats[2 * n_dims + d] = scale;
    }
}

__global__ __launch_bounds__(kThreads) void select_rows_kernel(const double *__restrict__ Z, long long ldz, long long n,
                                                               const int *__restrict__ rows, double *__restrict__ out, long long ldo) {
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t < n) out[(long long)blockIdx.y * ldo + t] = Z[(long long)rows[blockIdx.y] * ldz + t];
}

// grid (tiles x tiles, nk, kmax); labels null: every window (nk = kmax = 1).  out [nk][kmax][D][D]
__global__ __launch_bounds__(kThreads) void dimdist_kernel(const double *__restrict__ Z, long long ld, long long n, int D,
                                                           const int *__restrict__ labels, const int *__restrict__ ks, int kmax,
                                                           double *__restrict__ out) {
    __shared__ double A[kDimTile][kDimWin + 1], B[kDimTile][kDimWin + 1];
    __shared__ int live[kDimWin];
    const int nt = (D + kDimTile - 1) / kDimTile;
    const int bx = blockIdx.x % nt, by = blockIdx.x / nt, kidx = blockIdx.y, c = blockIdx.z;
    if (labels && c >= ks[kidx]) return;
    if (by > bx) return;
    const int tid = threadIdx.x, ti = tid / kDimTile, tj = tid % kDimTile;
    const int *lab = labels ? labels + (long long)kidx * n : nullptr;
    double acc = 0.0;
    for (long long t0 = 0; t0 < n; t0 += kDimWin) {
        __syncthreads();
        for (int e = tid; e < kDimTile * kDimWin; e += kThreads) {
            const int r = e / kDimWin, tt = e % kDimWin;
            const bool in = t0 + tt < n;
            const int ra = by * kDimTile + r, rb = bx * kDimTile + r;
            A[r][tt] = (in && ra < D) ? Z[(long long)ra * ld + t0 + tt] : 0.0;
            B[r][tt] = (in && rb < D) ? Z[(long long)rb * ld + t0 + tt] : 0.0;
        }
        if (tid < kDimWin) live[tid] = (t0 + tid < n) && (!lab || lab[t0 + tid] == c);
        __syncthreads();
        for (int tt = 0; tt < kDimWin; ++tt) {
            if (live[tt]) {
                const double df = A[ti][tt] - B[tj][tt];
                acc = fma(df, df, acc);
            }
        }
    }
    const int i = by * kDimTile + ti, j = bx * kDimTile + tj;
    if (i < D && j < D) {
        double *o = out + ((long long)kidx * kmax + c) * D * D;
        const double v = sqrt(acc);
        o[(long long)i * D + j] = v;
        o[(long long)j * D + i] = v;
    }
}

// grid (nk, kmax): colsum [nk][kmax][D] and the mean over the D (D - 1) / 2 pairs, pmean [nk][kmax]
__global__ __launch_bounds__(kThreads) void dimdist_reduce_kernel(const double *__restrict__ dist, int D, const int *__restrict__ ks,
                                                                  int kmax, double *__restrict__ colsum, double *__restrict__ pmean) {
    __shared__ double red[kThreads];
    const int kidx = blockIdx.x, c = blockIdx.y;
    if (ks && c >= ks[kidx]) return;
    const long long slot = (long long)kidx * kmax + c;
    const double *m = dist + slot * D * D;
    double upper = 0.0;
    for (int j = threadIdx.x; j < D; j += kThreads) {
        double s = 0.0, u = 0.0;
        for (int i = 0; i < D; ++i) {
            const double v = m[(long long)i * D + j];
            s += v;
            if (i < j) u += v;
        }
        colsum[slot * D + j] = s;
        upper += u;
    }
    upper = block_sum(upper, red);
    if (threadIdx.x == 0) pmean[slot] = upper / (0.5 * (double)D * (double)(D - 1));
}

// grid (window blocks, nk).  mode 0: a Lloyd assignment (k that are done are skipped): labels, d2 = the squared distance to
// the nearest centre, ints[kidx][0..31] += cluster sizes, ints[kidx][32] += changed labels.  mode 1: the last pass -- labels
// are re-assigned unless the run ended on unchanged labels, and d2 = the squared distance to the window's own centre.
// centers [nk][32][D]
template <int KP>
__global__ __launch_bounds__(kThreads) void assign_kernel(const double *__restrict__ Zk, long long ld, long long n, int D,
                                                          const int *__restrict__ ks, const double *__restrict__ centers,
                                                          const KmState *__restrict__ state, int mode, int *__restrict__ labels,
                                                          double *__restrict__ d2, int *__restrict__ ints) {
    __shared__ double cen[kDimChunk * KP];
    __shared__ int cnt[KP + 1];
    const int kidx = blockIdx.y, K = ks[kidx], tid = threadIdx.x;
    const KmState st = state[kidx];
    if (mode == 0 && st.done) return;
    const long long t = (long long)blockIdx.x * kThreads + tid;
    const bool live = t < n;
    const double *z = Zk + (live ? t : n - 1);
    const double *cb = centers + (long long)kidx * hmm::kMaxStates * D;
    if (tid <= KP) cnt[tid] = 0;
    double acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.0;
    for (int d0 = 0; d0 < D; d0 += kDimChunk) {
        const int nd = D - d0 < kDimChunk ? D - d0 : kDimChunk;
        __syncthreads();
        for (int e = tid; e < nd * KP; e += kThreads) {
            const int dd = e / KP, k = e % KP;
            cen[e] = k < K ? cb[(long long)k * D + d0 + dd] : 0.0;
        }
        __syncthreads();
        for (int dd = 0; dd < nd; ++dd) {
            const double zv = z[(long long)(d0 + dd) * ld];
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                const double df = zv - cen[dd * KP + k];
                acc[k] = fma(df, df, acc[k]);
            }
        }
    }
    int best = 0;
    double bv = acc[0];
#pragma unroll
    for (int k = 1; k < KP; ++k)
        if (k < K && acc[k] < bv) { bv = acc[k]; best = k; }
    if (live) {
        int *lp = labels + (long long)kidx * n + t;
        const int old = *lp;
        if (mode == 0 || !st.strict) {
            *lp = best;
            d2[(long long)kidx * n + t] = bv;
            if (mode == 0) {
                atomicAdd(&cnt[best], 1);
                if (best != old) atomicAdd(&cnt[KP], 1);
            }
        } else {
            double own = acc[0];
#pragma unroll
            for (int k = 1; k < KP; ++k)
                if (k == old) own = acc[k];
            d2[(long long)kidx * n + t] = own;
        }
    }
    if (mode != 0) return;
    __syncthreads();
    int *out = ints + kidx * (hmm::kMaxStates + 1);
    if (tid < K && cnt[tid]) atomicAdd(&out[tid], cnt[tid]);
    if (tid == KP && cnt[KP]) atomicAdd(&out[hmm::kMaxStates], cnt[KP]);
}

// grid (D, nk): sums [nk][32][D]
template <int KP>
__global__ __launch_bounds__(kThreads) void update_kernel(const double *__restrict__ Zk, long long ld, long long n, int D,
                                                          const int *__restrict__ ks, const KmState *__restrict__ state,
                                                          const int *__restrict__ labels, double *__restrict__ sums) {
    __shared__ double red[kThreads];
    const int d = blockIdx.x, kidx = blockIdx.y, K = ks[kidx];
    if (state[kidx].done) return;
    const double *z = Zk + (long long)d * ld;
    const int *lab = labels + (long long)kidx * n;
    double acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.0;
    for (long long t = threadIdx.x; t < n; t += kThreads) {
        const double zv = z[t];
        const int l = lab[t];
#pragma unroll
        for (int k = 0; k < KP; ++k) acc[k] += l == k ? zv : 0.0;
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        if (k < K) {
            const double s = block_sum(acc[k], red);
            if (threadIdx.x == 0) sums[((long long)kidx * hmm::kMaxStates + k) * D + d] = s;
        }
    }
}

// grid nk.  d2 of a window that an empty cluster takes is set to -1 (it is not taken twice)
__global__ __launch_bounds__(kThreads) void finish_kernel(const double *__restrict__ Zk, long long ld, long long n, int D,
                                                          const int *__restrict__ ks, const int *__restrict__ labels,
                                                          double *__restrict__ d2, const int *__restrict__ ints,
                                                          double *__restrict__ sums, double *__restrict__ centers,
                                                          KmState *__restrict__ state, double tol, int max_iter) {
    __shared__ double red[kThreads];
    __shared__ long long redi[kThreads];
    __shared__ int cnt[hmm::kMaxStates];
    const int kidx = blockIdx.x, K = ks[kidx], tid = threadIdx.x;
    if (state[kidx].done) return;
    const int *in = ints + kidx * (hmm::kMaxStates + 1);
    if (tid < hmm::kMaxStates) cnt[tid] = tid < K ? in[tid] : 0;
    __syncthreads();
    double *dk = d2 + (long long)kidx * n;
    double *sk = sums + (long long)kidx * hmm::kMaxStates * D;
    double *ck = centers + (long long)kidx * hmm::kMaxStates * D;
    int n_empty = 0;
    for (int e = 0; e < K; ++e) {
        if (cnt[e] != 0) continue;      // workgroup-uniform: cnt changes only between barriers
        ++n_empty;
        // the farthest window, lowest index among equal distances
        double bv = -2.0;
        long long bi = 0;
        for (long long t = tid; t < n; t += kThreads)
            if (dk[t] > bv) { bv = dk[t]; bi = t; }
        __syncthreads();
        red[tid] = bv;
        redi[tid] = bi;
        __syncthreads();
        for (int o = kThreads / 2; o > 0; o >>= 1) {
            if (tid < o && (red[tid + o] > red[tid] || (red[tid + o] == red[tid] && redi[tid + o] < redi[tid]))) {
                red[tid] = red[tid + o];
                redi[tid] = redi[tid + o];
            }
            __syncthreads();
        }
        const long long far = redi[0];
        const int old = labels[(long long)kidx * n + far];
        for (int d = tid; d < D; d += kThreads) {
            const double x = Zk[(long long)d * ld + far];
            sk[(long long)old * D + d] -= x;
            sk[(long long)e * D + d] = x;
        }
        __syncthreads();
        if (tid == 0) {
            dk[far] = -1.0;
            cnt[e] = 1;
            cnt[old] -= 1;
        }
        __threadfence_block();
        __syncthreads();
    }
    double sh = 0.0;
    for (int idx = tid; idx < K * D; idx += kThreads) {
        const int k = idx / D;
        const double c_old = ck[idx];
        const double c_new = cnt[k] > 0 ? sk[idx] / (double)cnt[k] : c_old;
        const double df = c_new - c_old;
        sh = fma(df, df, sh);
        ck[idx] = c_new;
    }
    sh = block_sum(sh, red);
    if (tid == 0) {
        KmState st = state[kidx];
        st.n_iter += 1;
        st.n_empty = n_empty;
        st.shift = sh;
        if (in[hmm::kMaxStates] == 0) { st.done = 1; st.strict = 1; }
        else if (sh <= tol || st.n_iter >= max_iter) st.done = 1;
        state[kidx] = st;
    }
}

// grid rows: out[row] = the sum of in[row][0 .. n - 1] in a fixed order
__global__ __launch_bounds__(kThreads) void row_sum_kernel(const double *__restrict__ in, long long n, double *__restrict__ out) {
    __shared__ double red[kThreads];
    const double *x = in + (long long)blockIdx.x * n;
    double s = 0.0;
    for (long long t = threadIdx.x; t < n; t += kThreads) s += x[t];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// out [n_pts][n]: squared distances of every window to the windows idx[0 .. n_pts - 1] (n_pts <= kMaxPoints)
__global__ __launch_bounds__(kThreads) void sqdist_points_kernel(const double *__restrict__ Zk, long long ld, long long n, int D,
                                                                 const long long *__restrict__ idx, int n_pts, double *__restrict__ out) {
    __shared__ double P[hmm::kMaxDims * kMaxPoints];
    const int tid = threadIdx.x;
    for (int e = tid; e < D * kMaxPoints; e += kThreads) {
        const int d = e / kMaxPoints, c = e % kMaxPoints;
        P[e] = c < n_pts ? Zk[(long long)d * ld + idx[c]] : 0.0;
    }
    __syncthreads();
    const long long t = (long long)blockIdx.x * kThreads + tid;
    if (t >= n) return;
    double acc[kMaxPoints];
#pragma unroll
    for (int c = 0; c < kMaxPoints; ++c) acc[c] = 0.0;
    for (int d = 0; d < D; ++d) {
        const double zv = Zk[(long long)d * ld + t];
#pragma unroll
        for (int c = 0; c < kMaxPoints; ++c) {
            const double df = zv - P[d * kMaxPoints + c];
            acc[c] = fma(df, df, acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < kMaxPoints; ++c)
        if (c < n_pts) out[(long long)c * n + t] = acc[c];
}

// grid n_pts: out [n_pts][D] = the windows idx[p]
__global__ __launch_bounds__(kThreads) void get_points_kernel(const double *__restrict__ Zk, long long ld, int D,
                                                              const long long *__restrict__ idx, double *__restrict__ out) {
    for (int d = threadIdx.x; d < D; d += kThreads) out[(long long)blockIdx.x * D + d] = Zk[(long long)d * ld + idx[blockIdx.x]];
}

// grid: the nb (nb + 1) / 2 tiles (bi <= bj), row after row.  binoff [nk + 1]: prefix sums of K^2; partial [tiles][binoff[nk]]
__global__ __launch_bounds__(kThreads) void pair_kernel(const double *__restrict__ Zk, long long ld, long long n, int D,
                                                        const int *__restrict__ labels, const int *__restrict__ ks, int nk, int nb,
                                                        const int *__restrict__ binoff, double *__restrict__ partial) {
    constexpr int T = kPairTile, R = T / 16;
    __shared__ double As[kPairDims][T], Bs[kPairDims][T];
    __shared__ double Tl[hmm::kMaxStates][T + 1];
    __shared__ int la[T], lb[T];
    int rem = blockIdx.x, bi = 0;
    while (rem >= nb - bi) { rem -= nb - bi; ++bi; }
    const int bj = bi + rem;
    const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
    const long long i0 = (long long)bi * T, j0 = (long long)bj * T;
    double acc[R][R];
#pragma unroll
    for (int u = 0; u < R; ++u)
#pragma unroll
        for (int v = 0; v < R; ++v) acc[u][v] = 0.0;
    for (int d0 = 0; d0 < D; d0 += kPairDims) {
        __syncthreads();
        for (int e = tid; e < kPairDims * T; e += kThreads) {
            const int dd = e / T, r = e % T;
            const bool din = d0 + dd < D;
            As[dd][r] = (din && i0 + r < n) ? Zk[(long long)(d0 + dd) * ld + i0 + r] : 0.0;
            Bs[dd][r] = (din && j0 + r < n) ? Zk[(long long)(d0 + dd) * ld + j0 + r] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int dd = 0; dd < kPairDims; ++dd) {
            double a[R], b[R];
#pragma unroll
            for (int u = 0; u < R; ++u) a[u] = As[dd][ty + 16 * u];
#pragma unroll
            for (int v = 0; v < R; ++v) b[v] = Bs[dd][tx + 16 * v];
#pragma unroll
            for (int u = 0; u < R; ++u)
#pragma unroll
                for (int v = 0; v < R; ++v) {
                    const double df = a[u] - b[v];
                    acc[u][v] = fma(df, df, acc[u][v]);
                }
        }
    }
#pragma unroll
    for (int u = 0; u < R; ++u)
#pragma unroll
        for (int v = 0; v < R; ++v) acc[u][v] = sqrt(acc[u][v]);
    const int nbins = binoff[nk];
    double *po = partial + (long long)blockIdx.x * nbins;
    for (int kidx = 0; kidx < nk; ++kidx) {
        const int K = ks[kidx];
        const int *lab = labels + (long long)kidx * n;
        __syncthreads();
        if (tid < T) la[tid] = i0 + tid < n ? lab[i0 + tid] : -1;
        else lb[tid - T] = j0 + (tid - T) < n ? lab[j0 + (tid - T)] : -1;
        __syncthreads();
        int lj[R];
#pragma unroll
        for (int v = 0; v < R; ++v) lj[v] = lb[tx + 16 * v];
        for (int c2 = 0; c2 < K; ++c2) {
#pragma unroll
            for (int u = 0; u < R; ++u) {
                double s = 0.0;
#pragma unroll
                for (int v = 0; v < R; ++v) s += lj[v] == c2 ? acc[u][v] : 0.0;
                s += __shfl_xor(s, 8, 16);
                s += __shfl_xor(s, 4, 16);
                s += __shfl_xor(s, 2, 16);
                s += __shfl_xor(s, 1, 16);
                if (tx == 0) Tl[c2][ty + 16 * u] = s;
            }
        }
        __syncthreads();
        for (int bin = tid; bin < K * K; bin += kThreads) {
            const int c = bin / K, c2 = bin % K;
            double s1 = 0.0, s2 = 0.0;
            for (int r = 0; r < T; ++r) {
                const int l = la[r];
                s1 += l == c ? Tl[c2][r] : 0.0;
                s2 += l == c2 ? Tl[c][r] : 0.0;
            }
            po[binoff[kidx] + bin] = bi == bj ? s1 : s1 + s2;
        }
    }
}

// grid (bin blocks, row chunks): out[chunk][bin] = the sum of in[r][bin] over the chunk's rows, in row order
__global__ __launch_bounds__(kThreads) void pair_reduce_kernel(const double *__restrict__ in, long long rows, int nbins, long long chunk,
                                                               double *__restrict__ out) {
    const int bin = blockIdx.x * kThreads + threadIdx.x;
    if (bin >= nbins) return;
    const long long r0 = (long long)blockIdx.y * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
    double s = 0.0;
    for (long long r = r0; r < r1; ++r) s += in[r * nbins + bin];
    out[(long long)blockIdx.y * nbins + bin] = s;
}

}  // namespace diar
}  // namespace paa
