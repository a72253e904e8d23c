// Speaker diarization of MANY clips at once (audioSegmentation.diarize_features_batch): the kernels of kernels_diar.hpp behind
// job records, plus k-means++ seeding on the device.  All FP64.  Every clip's matrix is a column range [col, col + n) of ONE
// feature-major matrix [n_dims][ld]; the kept feature rows of a clip are an index list (rows[rows_off .. rows_off + D - 1]), the
// rows are never compacted.  Every reduction runs in the order of its single-clip kernel, which depends on the clip's own n, D
// and k only, so clip i of a batch carries the bits of its own single call.
//
//  * standardize_kernel, dimdist_kernel / dimdist_reduce_kernel, assign_kernel / update_kernel / finish_kernel /
//    row_sum_kernel, pair_reduce_kernel: the bodies of kernels_diar.hpp; the clip, (clip, k) job or (job, cluster) slot comes
//    from blockIdx.y.
//  * seed_kernel: one workgroup per (clip, k) job runs all k greedy k-means++ steps from numbers the host drew up front.  The
//    loop of single calls forms three sums with NumPy, so their bits are NumPy's: closest.sum() and new.sum(axis = 1) (pairwise
//    summation -- serial below 8, eight strided accumulators up to 128, split at n / 2 rounded down to a multiple of 8 above --
//    of every chunk of 8192 elements, the chunks added serially; NumPy's 1-D sum is chunked too) and cumsum (serial).  The distance work
//    is spread over the workgroup; one lane per candidate walks the sums.
//  * pair_kernel: persistent workgroups over a host-built list of (clip, tile) items; all k of a clip share the pass.
#pragma once
#include "device_common.hpp"
#include "model_launch.hpp"

namespace paa {
namespace diarb {

using diar::BatchClip;
using diar::BatchJob;
using diar::BatchRed;
using diar::BatchSlot;
using diar::BatchTile;
using diar::KmState;

constexpr int kThreads = 256;
constexpr int kDimChunk = 32;
constexpr int kDimTile = 16;
constexpr int kDimWin = 64;
constexpr int kPairTile = diar::kBatchPairTile;
constexpr int kPairDims = 8;
constexpr int kSeedTrials = diar::kBatchTrials;   // 2 + int(ln 32) = 5 candidates at most
constexpr int kSeedDepth = 40;                    // pairwise-summation stack: one level per halving of n
constexpr long long kNpBlock = 128;               // NumPy's PW_BLOCKSIZE
constexpr long long kNpChunk = 8192;              // NumPy's reduction buffer, in elements

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

// grid (n_dims, clips); stats [clips][3][n_dims]: mean, variance, scale
__global__ __launch_bounds__(kThreads) void standardize_kernel(const double *__restrict__ M, long long ld,
                                                               const BatchClip *__restrict__ clips, int n_dims,
                                                               double *__restrict__ Z, double *__restrict__ stats_all) {
    __shared__ double red[kThreads];
    const int d = blockIdx.x;
    const BatchClip cl = clips[blockIdx.y];
    const long long n = cl.n;
    const double *x = M + (long long)d * ld + cl.col;
    double *stats = stats_all + (long long)blockIdx.y * 3 * n_dims;
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
    for (long long t = threadIdx.x; t < n; t += kThreads) Z[(long long)d * ld + cl.col + t] = (x[t] - mean) / scale;
    if (threadIdx.x == 0) {
        stats[d] = mean;
        stats[n_dims + d] = var;
        stats[2 * n_dims + d] = scale;
    }
}

// grid (tiles x tiles of the widest slot, slots): dist + slot.dist_off [D][D]
__global__ __launch_bounds__(kThreads) void dimdist_kernel(const double *__restrict__ Z, long long ld, const int *__restrict__ rows,
                                                           const BatchSlot *__restrict__ slots, const int *__restrict__ labels,
                                                           double *__restrict__ out) {
    __shared__ double A[kDimTile][kDimWin + 1], B[kDimTile][kDimWin + 1];
    __shared__ int live[kDimWin];
    const BatchSlot sl = slots[blockIdx.y];
    const int D = sl.D, c = sl.cluster;
    const long long n = sl.n;
    const int nt = (D + kDimTile - 1) / kDimTile;
    if ((int)blockIdx.x >= nt * nt) return;
    const int bx = blockIdx.x % nt, by = blockIdx.x / nt;
    if (by > bx) return;
    const int tid = threadIdx.x, ti = tid / kDimTile, tj = tid % kDimTile;
    const int *lab = sl.lab_off >= 0 ? labels + sl.lab_off : nullptr;
    const int *rw = sl.rows_off >= 0 ? rows + sl.rows_off : nullptr;
    const double *Zc = Z + sl.col;
    double acc = 0.0;
    for (long long t0 = 0; t0 < n; t0 += kDimWin) {
        __syncthreads();
        for (int e = tid; e < kDimTile * kDimWin; e += kThreads) {
            const int r = e / kDimWin, tt = e % kDimWin;
            const bool in = t0 + tt < n;
            const int ra = by * kDimTile + r, rb = bx * kDimTile + r;
            A[r][tt] = (in && ra < D) ? Zc[(long long)(rw ? rw[ra] : ra) * ld + t0 + tt] : 0.0;
            B[r][tt] = (in && rb < D) ? Zc[(long long)(rw ? rw[rb] : rb) * ld + t0 + tt] : 0.0;
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
        double *o = out + sl.dist_off;
        const double v = sqrt(acc);
        o[(long long)i * D + j] = v;
        o[(long long)j * D + i] = v;
    }
}

// grid slots: colsum + slot.sum_off [D] and pmean [slot]
__global__ __launch_bounds__(kThreads) void dimdist_reduce_kernel(const double *__restrict__ dist, const BatchSlot *__restrict__ slots,
                                                                  double *__restrict__ colsum, double *__restrict__ pmean) {
    __shared__ double red[kThreads];
    const BatchSlot sl = slots[blockIdx.x];
    const int D = sl.D;
    const double *m = dist + sl.dist_off;
    double upper = 0.0;
    for (int j = threadIdx.x; j < D; j += kThreads) {
        double s = 0.0, u = 0.0;
        for (int i = 0; i < D; ++i) {
            const double v = m[(long long)i * D + j];
            s += v;
            if (i < j) u += v;
        }
        colsum[sl.sum_off + j] = s;
        upper += u;
    }
    upper = block_sum(upper, red);
    if (threadIdx.x == 0) pmean[blockIdx.x] = upper / (0.5 * (double)D * (double)(D - 1));
}

// ---- NumPy's sums, one lane -------------------------------------------------------------------------------------------------
__device__ __forceinline__ double np_leaf(const double *__restrict__ a, long long n) {
    if (n < 8) {
        double res = 0.0;
        for (long long i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    long long i;
    for (i = 8; i < n - (n % 8); i += 8) {
        r0 += a[i + 0];
        r1 += a[i + 1];
        r2 += a[i + 2];
        r3 += a[i + 3];
        r4 += a[i + 4];
        r5 += a[i + 5];
        r6 += a[i + 6];
        r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += a[i];
    return res;
}

struct SeedStack {
    long long off[kSeedDepth], len[kSeedDepth];
    double val[kSeedDepth];
    int st[kSeedDepth];
};

// pairwise summation of a[0 .. n - 1] as NumPy's add.reduce runs it on a contiguous vector; the recursion is unrolled on `s`
__device__ double np_pairwise(const double *__restrict__ a, long long n, SeedStack &s) {
    int sp = 0;
    s.off[0] = 0;
    s.len[0] = n;
    s.st[0] = 0;
    double ret = 0.0;
    while (sp >= 0) {
        const long long o = s.off[sp], l = s.len[sp];
        long long h = l / 2;
        h -= h % 8;
        if (s.st[sp] == 0) {
            if (l <= kNpBlock) {
                ret = np_leaf(a + o, l);
                --sp;
            } else {
                s.st[sp] = 1;
                ++sp;
                s.off[sp] = o;
                s.len[sp] = h;
                s.st[sp] = 0;
            }
        } else if (s.st[sp] == 1) {
            s.val[sp] = ret;
            s.st[sp] = 2;
            ++sp;
            s.off[sp] = o + h;
            s.len[sp] = l - h;
            s.st[sp] = 0;
        } else {
            ret = s.val[sp] + ret;
            --sp;
        }
    }
    return ret;
}

// a contiguous vector or a row of a 2-D array summed along its last axis: the pairwise sum of every 8192 elements, added in order
__device__ double np_chunked(const double *__restrict__ a, long long n, SeedStack &s) {
    double res = 0.0;
    for (long long c0 = 0; c0 < n; c0 += kNpChunk) res += np_pairwise(a + c0, n - c0 < kNpChunk ? n - c0 : kNpChunk, s);
    return res;
}

// grid jobs.  closest + job.lab_off [n], tmp + job.tmp_off [trials][n]; centres + job.cen_off [k][D]; u + job.u_off
// [k - 1][trials].  A job whose centres the caller gave (seeded == 0) is left alone.
__global__ __launch_bounds__(kThreads) void seed_kernel(const double *__restrict__ Z, long long ld, const int *__restrict__ rows,
                                                        const BatchJob *__restrict__ jobs, const double *__restrict__ u,
                                                        double *closest_all, double *tmp_all, double *__restrict__ centers) {
    __shared__ double P[kSeedTrials][hmm::kMaxDims];
    __shared__ SeedStack stack[kSeedTrials];
    __shared__ long long cand[kSeedTrials];
    __shared__ double vals[kSeedTrials], csum[kSeedTrials];
    __shared__ int s_best;
    const BatchJob jb = jobs[blockIdx.x];
    if (!jb.seeded) return;
    const int tid = threadIdx.x, D = jb.D, K = jb.k, trials = jb.trials;
    const long long n = jb.n;
    const int *rw = rows + jb.rows_off;
    const double *Zc = Z + jb.col;
    double *closest = closest_all + jb.lab_off, *tmp = tmp_all + jb.tmp_off, *cen = centers + jb.cen_off;
    for (int d = tid; d < D; d += kThreads) {
        const double x = Zc[(long long)rw[d] * ld + jb.first];
        P[0][d] = x;
        cen[d] = x;
    }
    __syncthreads();
    for (long long t = tid; t < n; t += kThreads) {
        double acc = 0.0;
        for (int d = 0; d < D; ++d) {
            const double df = Zc[(long long)rw[d] * ld + t] - P[0][d];
            acc = fma(df, df, acc);
        }
        closest[t] = acc;
    }
    for (int step = 1; step < K; ++step) {
        __syncthreads();
        if (tid == 0) {
            const double pot = np_chunked(closest, n, stack[0]);
            for (int j = 0; j < trials; ++j) {
                vals[j] = u[jb.u_off + (long long)(step - 1) * trials + j] * pot;
                cand[j] = -1;
            }
            double c = 0.0;                                 // searchsorted(cumsum(closest), vals), side left
            for (long long t = 0; t < n; ++t) {
                c += closest[t];
                for (int j = 0; j < trials; ++j)
                    if (cand[j] < 0 && c >= vals[j]) cand[j] = t;
            }
            for (int j = 0; j < trials; ++j)
                if (cand[j] < 0) cand[j] = n - 1;
        }
        __syncthreads();
        for (int e = tid; e < kSeedTrials * D; e += kThreads) {        // rows past `trials` are zero: their distances are unused
            const int j = e / D, d = e % D;
            P[j][d] = j < trials ? Zc[(long long)rw[d] * ld + cand[j]] : 0.0;
        }
        __syncthreads();
        for (long long t = tid; t < n; t += kThreads) {
            double acc[kSeedTrials];
#pragma unroll
            for (int j = 0; j < kSeedTrials; ++j) acc[j] = 0.0;
            for (int d = 0; d < D; ++d) {
                const double zv = Zc[(long long)rw[d] * ld + t];
#pragma unroll
                for (int j = 0; j < kSeedTrials; ++j) {
                    const double df = zv - P[j][d];
                    acc[j] = fma(df, df, acc[j]);
                }
            }
            const double cl = closest[t];
#pragma unroll
            for (int j = 0; j < kSeedTrials; ++j)
                if (j < trials) tmp[(long long)j * n + t] = acc[j] < cl ? acc[j] : cl;
        }
        __syncthreads();
        if (tid < trials) csum[tid] = np_chunked(tmp + (long long)tid * n, n, stack[tid]);
        __syncthreads();
        if (tid == 0) {
            int best = 0;
            for (int j = 1; j < trials; ++j)
                if (csum[j] < csum[best]) best = j;
            s_best = best;
        }
        __syncthreads();
        const int best = s_best;
        for (int d = tid; d < D; d += kThreads) cen[(long long)step * D + d] = P[best][d];
        for (long long t = tid; t < n; t += kThreads) closest[t] = tmp[(long long)best * n + t];
    }
}

// ---- k-means over the job list ----------------------------------------------------------------------------------------------
// grid (window blocks of the longest job, jobs); see assign_kernel of kernels_diar.hpp.  ints [jobs][33]
template <int KP>
__global__ __launch_bounds__(kThreads) void assign_kernel(const double *__restrict__ Z, long long ld, const int *__restrict__ rows,
                                                          const BatchJob *__restrict__ jobs, const double *__restrict__ centers,
                                                          const KmState *__restrict__ state, int mode, int *__restrict__ labels,
                                                          double *__restrict__ d2, int *__restrict__ ints) {
    __shared__ double cen[kDimChunk * KP];
    __shared__ int cnt[KP + 1];
    const int kidx = blockIdx.y, tid = threadIdx.x;
    const BatchJob jb = jobs[kidx];
    const int K = jb.k, D = jb.D;
    const long long n = jb.n;
    if ((long long)blockIdx.x * kThreads >= n) return;
    const KmState st = state[kidx];
    if (mode == 0 && st.done) return;
    const long long t = (long long)blockIdx.x * kThreads + tid;
    const bool live = t < n;
    const double *z = Z + jb.col + (live ? t : n - 1);
    const int *rw = rows + jb.rows_off;
    const double *cb = centers + jb.cen_off;
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
            const double zv = z[(long long)rw[d0 + dd] * ld];
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
        int *lp = labels + jb.lab_off + t;
        const int old = *lp;
        if (mode == 0 || !st.strict) {
            *lp = best;
            d2[jb.lab_off + t] = bv;
            if (mode == 0) {
                atomicAdd(&cnt[best], 1);
                if (best != old) atomicAdd(&cnt[KP], 1);
            }
        } else {
            double own = acc[0];
#pragma unroll
            for (int k = 1; k < KP; ++k)
                if (k == old) own = acc[k];
            d2[jb.lab_off + t] = own;
        }
    }
    if (mode != 0) return;
    __syncthreads();
    int *out = ints + kidx * (hmm::kMaxStates + 1);
    if (tid < K && cnt[tid]) atomicAdd(&out[tid], cnt[tid]);
    if (tid == KP && cnt[KP]) atomicAdd(&out[hmm::kMaxStates], cnt[KP]);
}

// grid (dims of the widest job, jobs): sums + job.cen_off [k][D]
template <int KP>
__global__ __launch_bounds__(kThreads) void update_kernel(const double *__restrict__ Z, long long ld, const int *__restrict__ rows,
                                                          const BatchJob *__restrict__ jobs, const KmState *__restrict__ state,
                                                          const int *__restrict__ labels, double *__restrict__ sums) {
    __shared__ double red[kThreads];
    const int d = blockIdx.x, kidx = blockIdx.y;
    const BatchJob jb = jobs[kidx];
    const int K = jb.k, D = jb.D;
    const long long n = jb.n;
    if (d >= D || state[kidx].done) return;
    const double *z = Z + (long long)rows[jb.rows_off + d] * ld + jb.col;
    const int *lab = labels + jb.lab_off;
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
            if (threadIdx.x == 0) sums[jb.cen_off + (long long)k * D + d] = s;
        }
    }
}

// grid jobs; see finish_kernel of kernels_diar.hpp
__global__ __launch_bounds__(kThreads) void finish_kernel(const double *__restrict__ Z, long long ld, const int *__restrict__ rows,
                                                          const BatchJob *__restrict__ jobs, const int *__restrict__ labels,
                                                          double *__restrict__ d2, const int *__restrict__ ints,
                                                          double *__restrict__ sums, double *__restrict__ centers,
                                                          KmState *__restrict__ state, int max_iter) {
    __shared__ double red[kThreads];
    __shared__ long long redi[kThreads];
    __shared__ int cnt[hmm::kMaxStates];
    const int kidx = blockIdx.x, tid = threadIdx.x;
    const BatchJob jb = jobs[kidx];
    const int K = jb.k, D = jb.D;
    const long long n = jb.n;
    const double tol = jb.tol;
    if (state[kidx].done) return;
    const int *in = ints + kidx * (hmm::kMaxStates + 1);
    if (tid < hmm::kMaxStates) cnt[tid] = tid < K ? in[tid] : 0;
    __syncthreads();
    const int *rw = rows + jb.rows_off;
    const double *Zc = Z + jb.col;
    double *dk = d2 + jb.lab_off;
    double *sk = sums + jb.cen_off;
    double *ck = centers + jb.cen_off;
    int n_empty = 0;
    for (int e = 0; e < K; ++e) {
        if (cnt[e] != 0) continue;      // workgroup-uniform: cnt changes only between barriers
        ++n_empty;
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
        const int old = labels[jb.lab_off + far];
        for (int d = tid; d < D; d += kThreads) {
            const double x = Zc[(long long)rw[d] * ld + far];
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

// grid jobs: out[job] = the sum of d2 + job.lab_off [n] in the order of row_sum_kernel
__global__ __launch_bounds__(kThreads) void row_sum_kernel(const double *__restrict__ in, const BatchJob *__restrict__ jobs,
                                                           double *__restrict__ out) {
    __shared__ double red[kThreads];
    const BatchJob jb = jobs[blockIdx.x];
    const double *x = in + jb.lab_off;
    double s = 0.0;
    for (long long t = threadIdx.x; t < jb.n; t += kThreads) s += x[t];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---- cluster-pair distance sums ---------------------------------------------------------------------------------------------
// persistent workgroups over items [n_items] (tile bi <= bj of a clip); bintab + clip.bin_tab [nk + 1]: prefix sums of K^2;
// partial + item.part_off [bins of the clip]; labels of the clip's jobs: labels + clip.lab_off [nk][n]
__global__ __launch_bounds__(kThreads) void pair_kernel(const double *__restrict__ Z, long long ld, const int *__restrict__ rows,
                                                        const BatchClip *__restrict__ clips, const BatchJob *__restrict__ jobs,
                                                        const BatchTile *__restrict__ items, int n_items,
                                                        const int *__restrict__ labels, const int *__restrict__ bintab,
                                                        double *__restrict__ partial) {
    constexpr int T = kPairTile, R = T / 16;
    __shared__ double As[kPairDims][T], Bs[kPairDims][T];
    __shared__ double Tl[hmm::kMaxStates][T + 1];
    __shared__ int la[T], lb[T];
    const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const BatchTile it = items[item];
        const BatchClip cl = clips[it.clip];
        const int bi = it.bi, bj = it.bj, D = cl.D, nk = cl.nk;
        const long long n = cl.n;
        const int *rw = rows + cl.rows_off;
        const double *Zc = Z + cl.col;
        const int *binoff = bintab + cl.bin_tab;
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
                const long long row = din ? (long long)rw[d0 + dd] * ld : 0;
                As[dd][r] = (din && i0 + r < n) ? Zc[row + i0 + r] : 0.0;
                Bs[dd][r] = (din && j0 + r < n) ? Zc[row + j0 + r] : 0.0;
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
        double *po = partial + it.part_off;
        for (int kidx = 0; kidx < nk; ++kidx) {
            const int K = jobs[cl.first_job + kidx].k;
            const int *lab = labels + cl.lab_off + (long long)kidx * n;
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
}

// grid (bin blocks of the widest record, records): out + rec.out_off [bin] = the sum of in + rec.in_off [r][bin] over the
// record's rows, in row order
__global__ __launch_bounds__(kThreads) void pair_reduce_kernel(const double *__restrict__ in, const BatchRed *__restrict__ recs,
                                                               double *__restrict__ out) {
    const BatchRed rc = recs[blockIdx.y];
    const int bin = blockIdx.x * kThreads + threadIdx.x;
    if (bin >= rc.nbins) return;
    double s = 0.0;
    for (long long r = 0; r < rc.rows; ++r) s += in[rc.in_off + r * rc.nbins + bin];
    out[rc.out_off + bin] = s;
}

}  // namespace diarb
}  // namespace paa
