// Speaker diarization (kernels_diar.hpp: standardisation, feature-row distances, k-means, cluster-pair distance sums; and
// kernels_diarbatch.hpp: the same over a batch of clips, with k-means++ seeding on the device) -- own translation unit, see
// model_launch.hpp.
#include <cstdlib>
#include <cstring>

#include "model_launch.hpp"
#include "kernels_diar.hpp"
#include "kernels_diarbatch.hpp"

namespace paa {
namespace launch {

static int diar_status() { return hipGetLastError() == hipSuccess ? 0 : -1; }
static unsigned diar_blocks(long long n) { return (unsigned)((n + diar::kThreads - 1) / diar::kThreads); }
static bool diar_shape_ok(long long n, int D) { return n >= 1 && n <= 0x7fffffffLL / 64 && D >= 1 && D <= hmm::kMaxDims; }

int diar_standardize(const double *d_M, long long ldm, long long n, int n_dims, double *d_Z, long long ldz, double *d_stats,
                     hipStream_t stream) {
    if (!diar_shape_ok(n, n_dims) || ldm < n || ldz < n) return -1;
    hipLaunchKernelGGL(diar::standardize_kernel, dim3((unsigned)n_dims), dim3(diar::kThreads), 0, stream, d_M, ldm, n, n_dims, d_Z,
                       ldz, d_stats);
    return diar_status();
}

int diar_select_rows(const double *d_Z, long long ldz, long long n, const int *d_rows, int n_rows, double *d_out, long long ldo,
                     hipStream_t stream) {
    if (!diar_shape_ok(n, n_rows) || ldz < n || ldo < n) return -1;
    hipLaunchKernelGGL(diar::select_rows_kernel, dim3(diar_blocks(n), (unsigned)n_rows), dim3(diar::kThreads), 0, stream, d_Z, ldz, n,
                       d_rows, d_out, ldo);
    return diar_status();
}

int diar_dim_distances(const double *d_Z, long long ld, long long n, int D, const int *d_labels, const int *d_ks, int nk, int kmax,
                       double *d_dist, double *d_colsum, double *d_pmean, hipStream_t stream) {
    if (!diar_shape_ok(n, D) || ld < n || nk < 1 || kmax < 1 || kmax > hmm::kMaxStates) return -1;
    if (!d_labels && (nk != 1 || kmax != 1)) return -1;
    const int nt = (D + diar::kDimTile - 1) / diar::kDimTile;
    hipLaunchKernelGGL(diar::dimdist_kernel, dim3((unsigned)(nt * nt), (unsigned)nk, (unsigned)kmax), dim3(diar::kThreads), 0, stream,
                       d_Z, ld, n, D, d_labels, d_ks, kmax, d_dist);
    hipLaunchKernelGGL(diar::dimdist_reduce_kernel, dim3((unsigned)nk, (unsigned)kmax), dim3(diar::kThreads), 0, stream,
                       (const double *)d_dist, D, d_labels ? d_ks : nullptr, kmax, d_colsum, d_pmean);
    return diar_status();
}

template <int KP>
static void diar_assign(const double *d_Zk, long long ld, long long n, int D, const int *d_ks, int nk, const double *d_centers,
                        const diar::KmState *d_state, int mode, int *d_labels, double *d_d2, int *d_ints, hipStream_t stream) {
    hipLaunchKernelGGL(diar::assign_kernel<KP>, dim3(diar_blocks(n), (unsigned)nk), dim3(diar::kThreads), 0, stream, d_Zk, ld, n, D,
                       d_ks, d_centers, d_state, mode, d_labels, d_d2, d_ints);
}

static void diar_assign_any(int kmax, const double *d_Zk, long long ld, long long n, int D, const int *d_ks, int nk,
                            const double *d_centers, const diar::KmState *d_state, int mode, int *d_labels, double *d_d2, int *d_ints,
                            hipStream_t stream) {
    if (kmax <= 8) diar_assign<8>(d_Zk, ld, n, D, d_ks, nk, d_centers, d_state, mode, d_labels, d_d2, d_ints, stream);
    else if (kmax <= 16) diar_assign<16>(d_Zk, ld, n, D, d_ks, nk, d_centers, d_state, mode, d_labels, d_d2, d_ints, stream);
    else diar_assign<32>(d_Zk, ld, n, D, d_ks, nk, d_centers, d_state, mode, d_labels, d_d2, d_ints, stream);
}

int diar_kmeans_step(const double *d_Zk, long long ld, long long n, int D, const int *d_ks, int nk, int kmax, double *d_centers,
                     diar::KmState *d_state, int *d_labels, double *d_d2, int *d_ints, double *d_sums, double tol, int max_iter,
                     hipStream_t stream) {
    if (!diar_shape_ok(n, D) || ld < n || nk < 1 || kmax < 1 || kmax > hmm::kMaxStates) return -1;
    if (hipMemsetAsync(d_ints, 0, (size_t)nk * diar::kIntsPerK * sizeof(int), stream) != hipSuccess) return -1;
    diar_assign_any(kmax, d_Zk, ld, n, D, d_ks, nk, d_centers, d_state, 0, d_labels, d_d2, d_ints, stream);
    const dim3 grid((unsigned)D, (unsigned)nk), block(diar::kThreads);
    if (kmax <= 8)
        hipLaunchKernelGGL(diar::update_kernel<8>, grid, block, 0, stream, d_Zk, ld, n, D, d_ks, (const diar::KmState *)d_state,
                           (const int *)d_labels, d_sums);
    else if (kmax <= 16)
        hipLaunchKernelGGL(diar::update_kernel<16>, grid, block, 0, stream, d_Zk, ld, n, D, d_ks, (const diar::KmState *)d_state,
                           (const int *)d_labels, d_sums);
    else
        hipLaunchKernelGGL(diar::update_kernel<32>, grid, block, 0, stream, d_Zk, ld, n, D, d_ks, (const diar::KmState *)d_state,
                           (const int *)d_labels, d_sums);
    hipLaunchKernelGGL(diar::finish_kernel, dim3((unsigned)nk), block, 0, stream, d_Zk, ld, n, D, d_ks, (const int *)d_labels, d_d2,
                       (const int *)d_ints, d_sums, d_centers, d_state, tol, max_iter);
    return diar_status();
}

int diar_kmeans_last(const double *d_Zk, long long ld, long long n, int D, const int *d_ks, int nk, int kmax, const double *d_centers,
                     const diar::KmState *d_state, int *d_labels, double *d_d2, double *d_inertia, hipStream_t stream) {
    if (!diar_shape_ok(n, D) || ld < n || nk < 1 || kmax < 1 || kmax > hmm::kMaxStates) return -1;
    diar_assign_any(kmax, d_Zk, ld, n, D, d_ks, nk, d_centers, d_state, 1, d_labels, d_d2, nullptr, stream);
    hipLaunchKernelGGL(diar::row_sum_kernel, dim3((unsigned)nk), dim3(diar::kThreads), 0, stream, (const double *)d_d2, n, d_inertia);
    return diar_status();
}

int diar_sqdist_points(const double *d_Zk, long long ld, long long n, int D, const long long *d_idx, int n_pts, double *d_out,
                       hipStream_t stream) {
    if (!diar_shape_ok(n, D) || ld < n || n_pts < 1 || n_pts > diar::kMaxPoints) return -1;
    hipLaunchKernelGGL(diar::sqdist_points_kernel, dim3(diar_blocks(n)), dim3(diar::kThreads), 0, stream, d_Zk, ld, n, D, d_idx, n_pts,
                       d_out);
    return diar_status();
}

int diar_get_points(const double *d_Zk, long long ld, int D, const long long *d_idx, int n_pts, double *d_out, hipStream_t stream) {
    if (D < 1 || D > hmm::kMaxDims || n_pts < 1) return -1;
    hipLaunchKernelGGL(diar::get_points_kernel, dim3((unsigned)n_pts), dim3(diar::kThreads), 0, stream, d_Zk, ld, D, d_idx, d_out);
    return diar_status();
}

constexpr long long kPairChunk = 256;     // tiles added up by one thread of the first reduction stage

long long diar_pair_tiles(long long n) {
    const long long nb = (n + diar::kPairTile - 1) / diar::kPairTile;
    return nb * (nb + 1) / 2;
}

long long diar_pair_chunks(long long n) { return (diar_pair_tiles(n) + kPairChunk - 1) / kPairChunk; }

int diar_pair_sums(const double *d_Zk, long long ld, long long n, int D, const int *d_labels, const int *d_ks, int nk,
                   const int *d_binoff, int nbins, double *d_partial, double *d_stage, double *d_S, hipStream_t stream) {
    if (!diar_shape_ok(n, D) || ld < n || nk < 1 || nbins < 1) return -1;
    const long long nb = (n + diar::kPairTile - 1) / diar::kPairTile, tiles = diar_pair_tiles(n), chunks = diar_pair_chunks(n);
    if (tiles > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(diar::pair_kernel, dim3((unsigned)tiles), dim3(diar::kThreads), 0, stream, d_Zk, ld, n, D, d_labels, d_ks, nk,
                       (int)nb, d_binoff, d_partial);
    const unsigned bb = (unsigned)((nbins + diar::kThreads - 1) / diar::kThreads);
    hipLaunchKernelGGL(diar::pair_reduce_kernel, dim3(bb, (unsigned)chunks), dim3(diar::kThreads), 0, stream, (const double *)d_partial,
                       tiles, nbins, kPairChunk, d_stage);
    hipLaunchKernelGGL(diar::pair_reduce_kernel, dim3(bb, 1), dim3(diar::kThreads), 0, stream, (const double *)d_stage, chunks, nbins,
                       chunks, d_S);
    return diar_status();
}

// ---- the batch of clips (kernels_diarbatch.hpp) ------------------------------------------------------------------------------
static int diarb_status() { return hipGetLastError() == hipSuccess ? 0 : -1; }
static unsigned diarb_blocks(long long n) { return (unsigned)((n + diarb::kThreads - 1) / diarb::kThreads); }
constexpr int kDiarbMaxGridY = 65535;

int diarb_standardize(const double *d_M, long long ld, const diar::BatchClip *d_clips, int n_clips, int n_dims, double *d_Z,
                      double *d_stats, hipStream_t stream) {
    if (n_clips < 1 || n_clips > kDiarbMaxGridY || n_dims < 1 || n_dims > hmm::kMaxDims) return -1;
    hipLaunchKernelGGL(diarb::standardize_kernel, dim3((unsigned)n_dims, (unsigned)n_clips), dim3(diarb::kThreads), 0, stream, d_M, ld,
                       d_clips, n_dims, d_Z, d_stats);
    return diarb_status();
}

int diarb_dim_distances(const double *d_Z, long long ld, const int *d_rows, const diar::BatchSlot *d_slots, int n_slots, int max_D,
                        const int *d_labels, double *d_dist, double *d_colsum, double *d_pmean, hipStream_t stream) {
    if (n_slots < 1 || n_slots > kDiarbMaxGridY || max_D < 1 || max_D > hmm::kMaxDims) return -1;
    const int nt = (max_D + diarb::kDimTile - 1) / diarb::kDimTile;
    hipLaunchKernelGGL(diarb::dimdist_kernel, dim3((unsigned)(nt * nt), (unsigned)n_slots), dim3(diarb::kThreads), 0, stream, d_Z, ld,
                       d_rows, d_slots, d_labels, d_dist);
    hipLaunchKernelGGL(diarb::dimdist_reduce_kernel, dim3((unsigned)n_slots), dim3(diarb::kThreads), 0, stream, (const double *)d_dist,
                       d_slots, d_colsum, d_pmean);
    return diarb_status();
}

int diarb_seed(const double *d_Z, long long ld, const int *d_rows, const diar::BatchJob *d_jobs, int n_jobs, const double *d_u,
               double *d_closest, double *d_tmp, double *d_centers, hipStream_t stream) {
    if (n_jobs < 1) return -1;
    hipLaunchKernelGGL(diarb::seed_kernel, dim3((unsigned)n_jobs), dim3(diarb::kThreads), 0, stream, d_Z, ld, d_rows, d_jobs, d_u,
                       d_closest, d_tmp, d_centers);
    return diarb_status();
}

template <int KP>
static void diarb_assign(const double *d_Z, long long ld, const int *d_rows, const diar::BatchJob *d_jobs, int n_jobs, long long max_n,
                         const double *d_centers, const diar::KmState *d_state, int mode, int *d_labels, double *d_d2, int *d_ints,
                         hipStream_t stream) {
    hipLaunchKernelGGL(diarb::assign_kernel<KP>, dim3(diarb_blocks(max_n), (unsigned)n_jobs), dim3(diarb::kThreads), 0, stream, d_Z, ld,
                       d_rows, d_jobs, d_centers, d_state, mode, d_labels, d_d2, d_ints);
}

static void diarb_assign_any(int kmax, const double *d_Z, long long ld, const int *d_rows, const diar::BatchJob *d_jobs, int n_jobs,
                             long long max_n, const double *d_centers, const diar::KmState *d_state, int mode, int *d_labels,
                             double *d_d2, int *d_ints, hipStream_t stream) {
    if (kmax <= 8) diarb_assign<8>(d_Z, ld, d_rows, d_jobs, n_jobs, max_n, d_centers, d_state, mode, d_labels, d_d2, d_ints, stream);
    else if (kmax <= 16) diarb_assign<16>(d_Z, ld, d_rows, d_jobs, n_jobs, max_n, d_centers, d_state, mode, d_labels, d_d2, d_ints, stream);
    else diarb_assign<32>(d_Z, ld, d_rows, d_jobs, n_jobs, max_n, d_centers, d_state, mode, d_labels, d_d2, d_ints, stream);
}

static bool diarb_jobs_ok(int n_jobs, int kmax, long long max_n) {
    return n_jobs >= 1 && n_jobs <= kDiarbMaxGridY && kmax >= 1 && kmax <= hmm::kMaxStates && max_n >= 1 && max_n <= 0x7fffffffLL / 64;
}

int diarb_kmeans_step(const double *d_Z, long long ld, const int *d_rows, const diar::BatchJob *d_jobs, int n_jobs, int kmax,
                      long long max_n, int max_D, double *d_centers, diar::KmState *d_state, int *d_labels, double *d_d2,
                      int *d_ints, double *d_sums, int max_iter, hipStream_t stream) {
    if (!diarb_jobs_ok(n_jobs, kmax, max_n) || max_D < 1 || max_D > hmm::kMaxDims) return -1;
    if (hipMemsetAsync(d_ints, 0, (size_t)n_jobs * diar::kIntsPerK * sizeof(int), stream) != hipSuccess) return -1;
    diarb_assign_any(kmax, d_Z, ld, d_rows, d_jobs, n_jobs, max_n, d_centers, d_state, 0, d_labels, d_d2, d_ints, stream);
    const dim3 grid((unsigned)max_D, (unsigned)n_jobs), block(diarb::kThreads);
    if (kmax <= 8)
        hipLaunchKernelGGL(diarb::update_kernel<8>, grid, block, 0, stream, d_Z, ld, d_rows, d_jobs, (const diar::KmState *)d_state,
                           (const int *)d_labels, d_sums);
    else if (kmax <= 16)
        hipLaunchKernelGGL(diarb::update_kernel<16>, grid, block, 0, stream, d_Z, ld, d_rows, d_jobs, (const diar::KmState *)d_state,
                           (const int *)d_labels, d_sums);
    else
        hipLaunchKernelGGL(diarb::update_kernel<32>, grid, block, 0, stream, d_Z, ld, d_rows, d_jobs, (const diar::KmState *)d_state,
                           (const int *)d_labels, d_sums);
    hipLaunchKernelGGL(diarb::finish_kernel, dim3((unsigned)n_jobs), block, 0, stream, d_Z, ld, d_rows, d_jobs, (const int *)d_labels,
                       d_d2, (const int *)d_ints, d_sums, d_centers, d_state, max_iter);
    return diarb_status();
}

int diarb_kmeans_last(const double *d_Z, long long ld, const int *d_rows, const diar::BatchJob *d_jobs, int n_jobs, int kmax,
                      long long max_n, const double *d_centers, const diar::KmState *d_state, int *d_labels, double *d_d2,
                      double *d_inertia, hipStream_t stream) {
    if (!diarb_jobs_ok(n_jobs, kmax, max_n)) return -1;
    diarb_assign_any(kmax, d_Z, ld, d_rows, d_jobs, n_jobs, max_n, d_centers, d_state, 1, d_labels, d_d2, nullptr, stream);
    hipLaunchKernelGGL(diarb::row_sum_kernel, dim3((unsigned)n_jobs), dim3(diarb::kThreads), 0, stream, (const double *)d_d2, d_jobs,
                       d_inertia);
    return diarb_status();
}

int diarb_pair_sums(const double *d_Z, long long ld, const int *d_rows, const diar::BatchClip *d_clips, const diar::BatchJob *d_jobs,
                    const diar::BatchTile *d_items, int n_items, const int *d_labels, const int *d_bintab, double *d_partial,
                    const diar::BatchRed *d_red1, int n_red1, double *d_stage, const diar::BatchRed *d_red2, int n_red2,
                    double *d_S, int max_bins, int workgroups, hipStream_t stream) {
    if (n_items < 1 || n_red1 < 1 || n_red1 > kDiarbMaxGridY || n_red2 < 1 || n_red2 > kDiarbMaxGridY || max_bins < 1 || workgroups < 1)
        return -1;
    const int wgs = n_items < workgroups ? n_items : workgroups;
    hipLaunchKernelGGL(diarb::pair_kernel, dim3((unsigned)wgs), dim3(diarb::kThreads), 0, stream, d_Z, ld, d_rows, d_clips, d_jobs,
                       d_items, n_items, d_labels, d_bintab, d_partial);
    const unsigned bb = (unsigned)((max_bins + diarb::kThreads - 1) / diarb::kThreads);
    hipLaunchKernelGGL(diarb::pair_reduce_kernel, dim3(bb, (unsigned)n_red1), dim3(diarb::kThreads), 0, stream,
                       (const double *)d_partial, d_red1, d_stage);
    hipLaunchKernelGGL(diarb::pair_reduce_kernel, dim3(bb, (unsigned)n_red2), dim3(diarb::kThreads), 0, stream,
                       (const double *)d_stage, d_red2, d_S);
    return diarb_status();
}

}  // namespace launch
}  // namespace paa
