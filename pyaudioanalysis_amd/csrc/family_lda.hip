// Linear discriminant analysis of speaker diarization (kernels_lda.hpp: class statistics, within-class Gram matrix,
// projection) -- own translation unit, see model_launch.hpp.
#include <cstdlib>
#include <cstring>

#include "model_launch.hpp"
#include "kernels_lda.hpp"

namespace paa {
namespace launch {

static int lda_status() { return hipGetLastError() == hipSuccess ? 0 : -1; }
static unsigned lda_blocks(long long n) { return (unsigned)((n + lda::kThreads - 1) / lda::kThreads); }
static bool lda_shape_ok(long long n, int D) { return n >= 1 && n <= 0x7fffffffLL / 64 && D >= 1 && D <= hmm::kMaxDims; }

int lda_class_stats(const double *d_X, long long ld, long long n, int D, const long long *d_off, long long C, double *d_means,
                    double *d_dev, double *d_sq, double *d_std, hipStream_t stream) {
    if (!lda_shape_ok(n, D) || ld < n || C < 1 || C > n) return -1;
    hipLaunchKernelGGL(lda::class_stats_kernel, dim3((unsigned)C, (unsigned)((D + 3) / 4)), dim3(lda::kThreads), 0, stream, d_X, ld, D,
                       d_off, d_means, d_dev, d_sq);
    hipLaunchKernelGGL(lda::pool_kernel, dim3(lda_blocks(D)), dim3(lda::kThreads), 0, stream, (const double *)d_dev,
                       (const double *)d_sq, C, D, n, d_std);
    return lda_status();
}

long long lda_gram_chunks(long long n) { return (n + lda::kGramChunk - 1) / lda::kGramChunk; }

int lda_within_gram(const double *d_X, long long ld, long long n, int D, const long long *d_off, long long C, const double *d_means,
                    const double *d_rscale, int *d_cls, double *d_partial, double *d_G, hipStream_t stream) {
    if (!lda_shape_ok(n, D) || ld < n || C < 1 || C > n) return -1;
    const int tiles = (D + lda::kGramTile - 1) / lda::kGramTile;
    const long long chunks = lda_gram_chunks(n);
    if (chunks > 65535) return -1;
    hipLaunchKernelGGL(lda::window_class_kernel, dim3(lda_blocks(n)), dim3(lda::kThreads), 0, stream, d_off, C, n, d_cls);
    hipLaunchKernelGGL(lda::gram_kernel, dim3((unsigned)(tiles * (tiles + 1) / 2), (unsigned)chunks), dim3(lda::kThreads), 0, stream,
                       d_X, ld, n, D, (const int *)d_cls, d_means, d_rscale, d_partial);
    hipLaunchKernelGGL(lda::gram_reduce_kernel, dim3(lda_blocks((long long)D * D)), dim3(lda::kThreads), 0, stream,
                       (const double *)d_partial, chunks, D, d_G);
    return lda_status();
}

int lda_project(const double *d_X, long long ld, long long n, int D, const double *d_xbar, const double *d_S, int n_out, double *d_Y,
                long long ldy, hipStream_t stream) {
    if (!lda_shape_ok(n, D) || ld < n || ldy < n || n_out < 1 || n_out > D) return -1;
    hipLaunchKernelGGL(lda::project_kernel, dim3(lda_blocks(n), (unsigned)((n_out + lda::kProjOut - 1) / lda::kProjOut)),
                       dim3(lda::kThreads), 0, stream, d_X, ld, n, D, d_xbar, d_S, n_out, d_Y, ldy);
    return lda_status();
}

}  // namespace launch
}  // namespace paa
