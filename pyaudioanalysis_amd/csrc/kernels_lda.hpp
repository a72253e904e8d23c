// Linear discriminant analysis of speaker diarization (audioSegmentation.speaker_diarization, :880-934, lda_dim > 0): the
// O(n) parts of scikit-learn's svd-solver LinearDiscriminantAnalysis.  All FP64; every matrix is feature-major
// [n_dims][ld], window t in column t.  Classes are CONTIGUOUS runs of windows: class c = windows off[c] .. off[c + 1] - 1.
//
//  * class_stats_kernel: one wave per (class, feature row): the run's mean (lane partials in window order, fixed
//    shuffle tree), then -- second pass over the run -- the sum of the deviations and of their squares.
//    pool_kernel: thread per feature row adds the classes' sums in class order: the pooled within-class deviation
//    (corrected two-pass form; zero -> 1, NaN propagates).
//  * window_class_kernel: cls [n] = the class of every window (binary search in off).
//  * gram_kernel: partial Gram matrices of Xs = (X - mean of the window's class) * rscale per feature row, centred and
//    scaled on the load path (Xs never exists in HBM).  Workgroup = (64 x 64 tile of G on or above the diagonal, chunk of
//    kGramChunk windows); the two 64-row panels of a step of kGramStep windows are staged in LDS; wave w owns the
//    32 x 32 block (w >> 1, w & 1) of the tile as 2 x 2 blocks of v_mfma_f64_16x16x4_f64 (32 accumulator registers; the
//    vector unit would need the same 16 accumulators per lane plus broadcast operands -- the matrix form is the one with
//    the lower register pressure, the rates are equal on gfx950).  Blocks wholly below the diagonal or wholly in the padding
//    are skipped.  The windows of a chunk are consumed in order, so a partial is a fixed-order sum.
//    gram_reduce_kernel: G[a][b] = the chunks' partials of cell (min, max) added in chunk order -- the mirror image is
//    the same bits, no floating-point atomics anywhere.
//  * project_kernel: Y[j][t] = sum_d (X[d][t] - xbar[d]) S[d][j], d ascending; thread per window, kProjOut outputs each.
#pragma once
#include "device_common.hpp"
#include "model_launch.hpp"

namespace paa {
namespace lda {

constexpr int kThreads = 256;
constexpr int kGramTile = 64;         // feature rows per tile side
constexpr int kGramStep = 32;         // windows staged per step
constexpr int kGramPitch = 34;        // LDS row pitch in doubles: the 16 rows x 2 windows a half-wave reads hit 32 different bank pairs
constexpr int kGramChunk = 1024;      // windows per partial (fixed: the result does not depend on the device)
constexpr int kProjOut = 8;           // outputs per thread of project_kernel

// grid (n_classes, ceil(D / 4)); wave w of the block: feature row 4 blockIdx.y + w.  means / dev / sq [C][D]
__global__ __launch_bounds__(kThreads) void class_stats_kernel(const double *__restrict__ X, long long ld, int D,
                                                               const long long *__restrict__ off, double *__restrict__ means,
                                                               double *__restrict__ dev, double *__restrict__ sq) {
    const int lane = threadIdx.x & 63, d = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (d >= D) return;                                     // (whole waves leave; no barrier below)
    const long long c = blockIdx.x, t0 = off[c], t1 = off[c + 1];
    const double *x = X + (long long)d * ld;
    double s = 0.0;
    for (long long t = t0 + lane; t < t1; t += 64) s += x[t];
    const double mean = wsum(s) / (double)(t1 - t0);
    double e = 0.0, q = 0.0;
    for (long long t = t0 + lane; t < t1; t += 64) {
        const double df = x[t] - mean;
        e += df;
        q = fma(df, df, q);
    }
    e = wsum(e);
    q = wsum(q);
    if (lane == 0) {
        means[c * D + d] = mean;
        dev[c * D + d] = e;
        sq[c * D + d] = q;
    }
}

__global__ __launch_bounds__(kThreads) void pool_kernel(const double *__restrict__ dev, const double *__restrict__ sq, long long C,
                                                        int D, long long n, double *__restrict__ std_out) {
    const int d = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (d >= D) return;
    double e = 0.0, q = 0.0;
    for (long long c = 0; c < C; ++c) {
        e += dev[c * D + d];
        q += sq[c * D + d];
    }
    const double var = (q - e * e / (double)n) / (double)n;
    // zero (a constant row; also a variance that rounding left below zero) -> 1; a NaN stays a NaN, as in scikit-learn
    std_out[d] = var != var ? var : (var > 0.0 ? sqrt(var) : 1.0);
}

__global__ __launch_bounds__(kThreads) void window_class_kernel(const long long *__restrict__ off, long long C, long long n,
                                                                int *__restrict__ cls) {
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    long long lo = 0, hi = C - 1;                           // the last c with off[c] <= t
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (off[mid] <= t) lo = mid; else hi = mid - 1;
    }
    cls[t] = (int)lo;
}

typedef double f64x4 __attribute__((ext_vector_type(4)));

// row-major enumeration of the tiles on and above the diagonal
__device__ __forceinline__ void tri_tile(int t, int tiles, int &ti, int &tj) {
    int r = 0;
    while (t >= tiles - r) {
        t -= tiles - r;
        ++r;
    }
    ti = r;
    tj = r + t;
}

// grid (tiles (tiles + 1) / 2, chunks); partial [chunks][D][D].  Four workgroups per CU (the LDS bound: 34 KB each), i.e. four
// waves per SIMD and 128 registers, accumulators included
__global__ __launch_bounds__(kThreads, 4) void gram_kernel(const double *__restrict__ X, long long ld, long long n, int D,
                                                        const int *__restrict__ cls, const double *__restrict__ means,
                                                        const double *__restrict__ rscale, double *__restrict__ partial) {
    __shared__ double pa[kGramTile * kGramPitch], pb[kGramTile * kGramPitch];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tiles = (D + kGramTile - 1) / kGramTile;
    int ti, tj;
    tri_tile((int)blockIdx.x, tiles, ti, tj);
    const int a0 = ti * kGramTile, b0 = tj * kGramTile;
    const int wi = 32 * (wave >> 1), wj = 32 * (wave & 1);
    // the wave's block is needed when it reaches the diagonal or lies above it and holds a feature row and column
    const bool active = a0 + wi <= b0 + wj && a0 + wi < D && b0 + wj < D;
    const bool diag = ti == tj;
    const long long chunk = blockIdx.y, t_begin = chunk * kGramChunk, t_end = min(n, t_begin + kGramChunk);
    const int col = threadIdx.x & 31, row0 = threadIdx.x >> 5;       // staging: window col, rows row0 + 8 q
    const int lm = lane & 15, lk = lane >> 4;
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (long long s0 = t_begin; s0 < t_end; s0 += kGramStep) {
        const long long t = s0 + col;
        const bool live = t < t_end;
        const long long c = live ? (long long)cls[t] : 0;
        __syncthreads();                                    // the previous step's panels are consumed
#pragma unroll
        for (int q = 0; q < kGramTile / 8; ++q) {
            const int r = row0 + 8 * q, da = a0 + r, db = b0 + r;
            double va = 0.0, vb = 0.0;
            if (live && da < D) va = (X[(long long)da * ld + t] - means[c * D + da]) * rscale[da];
            pa[r * kGramPitch + col] = va;
            if (!diag) {
                if (live && db < D) vb = (X[(long long)db * ld + t] - means[c * D + db]) * rscale[db];
                pb[r * kGramPitch + col] = vb;
            }
        }
        __syncthreads();
        if (active) {
            const double *B = diag ? pa : pb;
            // operand maps of v_mfma_f64_16x16x4_f64: A[m = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15]
#pragma unroll
            for (int kk = 0; kk < kGramStep; kk += 4) {
                double av[2], bv[2];
#pragma unroll
                for (int a = 0; a < 2; ++a) av[a] = pa[(wi + 16 * a + lm) * kGramPitch + kk + lk];
#pragma unroll
                for (int b = 0; b < 2; ++b) bv[b] = B[(wj + 16 * b + lm) * kGramPitch + kk + lk];
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
            }
        }
    }
    if (!active) return;
    // C/D map of the f64 form: column = lane & 15, row = (lane >> 4) + 4 * reg
    double *out = partial + chunk * (long long)D * D;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int da = a0 + wi + 16 * a + 4 * r + lk, db = b0 + wj + 16 * b + lm;
                if (da < D && db < D) out[(long long)da * D + db] = acc[a][b][r];
            }
}

// thread per cell of G [D][D]
__global__ __launch_bounds__(kThreads) void gram_reduce_kernel(const double *__restrict__ partial, long long chunks, int D,
                                                               double *__restrict__ G) {
    const long long cell = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (cell >= (long long)D * D) return;
    const int a = (int)(cell / D), b = (int)(cell % D);
    const long long src = (long long)min(a, b) * D + max(a, b);
    double s = 0.0;
    for (long long c = 0; c < chunks; ++c) s += partial[c * (long long)D * D + src];
    G[cell] = s;
}

// grid (ceil(n / 256), ceil(n_out / kProjOut)); S [D][n_out]
__global__ __launch_bounds__(kThreads) void project_kernel(const double *__restrict__ X, long long ld, long long n, int D,
                                                           const double *__restrict__ xbar, const double *__restrict__ S, int n_out,
                                                           double *__restrict__ Y, long long ldy) {
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int j0 = (int)blockIdx.y * kProjOut, nj = min(kProjOut, n_out - j0);
    if (t >= n) return;
    double acc[kProjOut];
#pragma unroll
    for (int q = 0; q < kProjOut; ++q) acc[q] = 0.0;
    for (int d = 0; d < D; ++d) {
        const double v = X[(long long)d * ld + t] - xbar[d];
        const double *s = S + (long long)d * n_out + j0;
#pragma unroll
        for (int q = 0; q < kProjOut; ++q) acc[q] = fma(v, s[q < nj ? q : 0], acc[q]);
    }
#pragma unroll
    for (int q = 0; q < kProjOut; ++q)
        if (q < nj) Y[(long long)(j0 + q) * ldy + t] = acc[q];
}

}  // namespace lda
}  // namespace paa
