// Self-similarity matrix and thumbnail filter for a BATCH of ragged clips (music_thumbnailing over a collection): the kernels
// of kernels_sim.hpp restated over host-built lists, so that the Gram tiles, the diagonal blocks and the folds of a thousand
// songs are one launch each.  Clip c has T_c vectors and R_c = T_c - M + 1 filtered rows; every per-clip array sits at a 64-bit
// offset of its own (SimClip / ThumbClip).  The contract is bit-equality with the single-clip kernels: same arithmetic, same
// order, same fold trees.
//
//   sim_row_stats_batch : block = (clip, feature row); sim_row_stats_kernel's two passes
//   sim_normalize_batch : grid (clip, column block); Z_c [dims_pad][ldz_c] with zero padding, 1/|z_t|
//   sim_gram_batch      : persistent workgroups over the tile list (clip, ti <= tj), clip-major; sim_gram_kernel's tile body,
//                         fused epilogue, unit diagonal and transposed second store -- a tile's bits do not depend on the
//                         workgroup that computes it
//   thumb_diag_batch    : one block per list entry (clip, bx, by); only blocks that hold a cell are listed.  A clip's minima
//                         and arg-max candidates sit in ITS segment of the candidate scratch, at the slot by * gx + bx the
//                         single call uses
//   thumb_min_batch /
//   thumb_argmax_batch  : one workgroup per clip; slots of unlisted blocks are not read, they count as what the single kernel
//                         writes for a block without cells (+inf / no candidate), so the fold trees are the single call's
//   thumb_fill_batch    : grid (list of (clip, row block), column block)
//   thumb_grow_batch    : one thread per clip walks audioSegmentation._grow_thumbnail (audioSegmentation.py:1167-1182) on the
//                         clip's filtered matrix: the host needs no matrix at all
#pragma once
#include "kernels_sim.hpp"

namespace paa {
namespace simb {

struct SimClip {            // offsets in doubles
    long long feat_off;     // [n_dims][ld_in] feature matrix in the feature buffer
    long long ld_in;
    long long n;            // T_c
    long long ldz;          // T_c rounded up to kSimTile
    long long z_off;        // Z_c [dims_pad][ldz] in the Z scratch
    long long aux_off;      // mean [n_dims] | scale [n_dims] | 1/|z| [ldz] in the small scratch
    long long sim_off;      // [n][n] matrix in the similarity buffer
};
struct SimTile { int clip, ti, tj, pad; };

struct ThumbClip {          // offsets in doubles (8-byte words for cand_off)
    long long sim_off, filt_off;
    long long cand_off;     // block_min [n_blk] | min | cand_val [n_blk] | cand_idx [n_blk] | best, n_blk = gx * gy
    long long n, R, lim_lo, lim_hi;
    int gx, gy;             // thumb_diag's grid of the single call: ceil(R / 256) x ceil(R / kDiagRun)
};
struct ThumbBlock { int clip, bx, by, pad; };

// block (bx, by) of thumb_diag holds a cell: its smallest diagonal offset starts inside the matrix
__host__ __device__ __forceinline__ bool diag_block_live(long long bx, long long by, long long R) {
    return 256 * bx + (long long)kDiagRun * by < R;
}

// block = clip * n_dims + feature row
__global__ __launch_bounds__(256) void sim_row_stats_batch_kernel(const double *__restrict__ feats,
                                                                   const SimClip *__restrict__ clips, int n_dims,
                                                                   double *__restrict__ aux) {
    __shared__ double red[2][4];
    const SimClip c = clips[blockIdx.x / (unsigned)n_dims];
    const int d_row = (int)(blockIdx.x % (unsigned)n_dims);
    const long long n = c.n;
    const double *row = feats + c.feat_off + (long long)d_row * c.ld_in;
    double *mean_out = aux + c.aux_off, *scale_out = mean_out + n_dims;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s = 0.0;
    for (long long t = threadIdx.x; t < n; t += 256) s += row[t];
    s = wsum(s);
    if (lane == 0) red[0][wave] = s;
    __syncthreads();
    const double mean = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (double)n;
    __syncthreads();
    double cs = 0.0, q = 0.0;
    for (long long t = threadIdx.x; t < n; t += 256) {
        const double d = row[t] - mean;
        cs += d;
        q = fma(d, d, q);
    }
    cs = wsum(cs);
    q = wsum(q);
    if (lane == 0) { red[0][wave] = cs; red[1][wave] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double corr = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        const double ss = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        const double nn = (double)n;
        const double var = (ss - corr * corr / nn) / nn;
        const double ub = nn * kEps * var + (nn * mean * kEps) * (nn * mean * kEps);
        mean_out[d_row] = mean;
        scale_out[d_row] = (var <= ub) ? 1.0 : sqrt(var);
    }
}

// grid (clip, column block): thread per column of Z_c, padding columns included
__global__ __launch_bounds__(256) void sim_normalize_batch_kernel(const double *__restrict__ feats,
                                                                   const SimClip *__restrict__ clips, int n_dims,
                                                                   int dims_pad, double *__restrict__ aux,
                                                                   double *__restrict__ zbuf) {
    const SimClip c = clips[blockIdx.x];
    const long long t = (long long)blockIdx.y * 256 + threadIdx.x;
    const long long n = c.n, ld = c.ldz, ld_in = c.ld_in;
    if (t >= ld) return;
    const double *x = feats + c.feat_off;
    const double *mean = aux + c.aux_off, *scale = mean + n_dims;
    double *z = zbuf + c.z_off, *norm = aux + c.aux_off + 2 * n_dims;
    double acc = 0.0;
    for (int d = 0; d < dims_pad; ++d) {
        double v = 0.0;
        if (d < n_dims && t < n) {
            v = (x[(long long)d * ld_in + t] - mean[d]) / scale[d];
            acc = fma(v, v, acc);
        }
        z[(long long)d * ld + t] = v;
    }
    norm[t] = 1.0 / sqrt(acc);
}

// grid = min(list length, 2 per CU) persistent workgroups of 512 threads, dynamic LDS as sim_gram_kernel.  The tile body and the
// epilogue are sim_gram_kernel's, statement for statement; what changes per tile is where Z, the norms and the output start.
__global__ __launch_bounds__(512, 4) void sim_gram_batch_kernel(const double *__restrict__ zbuf, int dims_pad, int n_dims,
                                                                 const SimClip *__restrict__ clips,
                                                                 const SimTile *__restrict__ tiles, long long n_tiles,
                                                                 const double *__restrict__ aux,
                                                                 double *__restrict__ simbuf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char simb_smem[];
    double *pa = reinterpret_cast<double *>(simb_smem);             // [kSimChunk][kSimPitch]: columns i0 .. i0+127
    double *pb = pa + kSimChunk * kSimPitch;                        // columns j0 .. j0+127
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wi = 32 * (wave >> 1), wj = 64 * (wave & 1);
    const int lm = lane & 15, lk = lane >> 4;
    double *nrm = pb + kSimChunk * kSimPitch;                       // [256]: 1/|z| of the tile's 128 rows, then its 128 columns
    double *tr = pa + wave * (16 * 17);                             // the wave's transposition scratch
    constexpr int PF = kSimChunk * 64 / 512;
    double fax[PF], fay[PF], fbx[PF], fby[PF];
    const int prow = threadIdx.x >> 6, pc2 = threadIdx.x & 63;
    // the tile in hand: its clip's Z, pitch, vector count, norms and output (uniform: scalar registers)
    const double *z = zbuf, *rnorm = aux;
    double *sim = simbuf;
    long long ld = kSimTile, n = 0, ti = 0, tj = 0;
#define PAA_SIMB_TILE(t_)                                                                                    \
    {                                                                                                        \
        const SimTile tl_ = tiles[t_];                                                                       \
        const SimClip *cl_ = clips + tl_.clip;                                                               \
        z = zbuf + cl_->z_off; ld = cl_->ldz; n = cl_->n;                                                    \
        rnorm = aux + cl_->aux_off + 2 * n_dims; sim = simbuf + cl_->sim_off;                                \
        ti = tl_.ti; tj = tl_.tj;                                                                            \
    }
#define PAA_SIMB_FETCH(k0_, i0_, j0_)                                                                        \
    _Pragma("unroll") for (int q = 0; q < PF; ++q) {                                                         \
        const long long grow = min((k0_) + prow + 8 * q, dims_pad - 1);                                      \
        const double2 ta_ = *reinterpret_cast<const double2 *>(z + grow * ld + (i0_) + 2 * pc2);             \
        const double2 tb_ = *reinterpret_cast<const double2 *>(z + grow * ld + (j0_) + 2 * pc2);             \
        fax[q] = ta_.x; fay[q] = ta_.y; fbx[q] = tb_.x; fby[q] = tb_.y;                                      \
    }
    if ((long long)blockIdx.x < n_tiles) {
        PAA_SIMB_TILE(blockIdx.x)
        PAA_SIMB_FETCH(0, ti * kSimTile, tj * kSimTile)
    }
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long i0 = ti * kSimTile, j0 = tj * kSimTile;
    const bool mirror = ti != tj;
    f64x4 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < dims_pad; k0 += kSimChunk) {
        const int kc = min(kSimChunk, dims_pad - k0);                // multiple of 4
        __syncthreads();                                             // previous chunk (or transposition scratch) consumed
#pragma unroll
        for (int q = 0; q < PF; ++q) {
            *reinterpret_cast<double2 *>(pa + (prow + 8 * q) * kSimPitch + 2 * pc2) = make_double2(fax[q], fay[q]);
            *reinterpret_cast<double2 *>(pb + (prow + 8 * q) * kSimPitch + 2 * pc2) = make_double2(fbx[q], fby[q]);
        }
        if (k0 == 0) {
            int tn = threadIdx.x;
            asm volatile("" : "+v"(tn));
            if (tn < 256) nrm[tn] = rnorm[(tn < 128 ? i0 : j0 - 128) + tn];
        }
        __syncthreads();
        if (k0 + kSimChunk < dims_pad) PAA_SIMB_FETCH(k0 + kSimChunk, i0, j0)
        for (int kk = 0; kk < kc; kk += 4) {
            const double *ra = pa + (kk + lk) * kSimPitch + wi + lm;
            const double *rb = pb + (kk + lk) * kSimPitch + wj + lm;
            double av[2], bv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) bv[q] = rb[16 * q];
            av[0] = ra[0];
            av[1] = ra[16];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
    }
    if (mirror) __syncthreads();                  // every wave is done with the panels: their LDS becomes the scratch
    int elm = lm, elk = lk, ewi = wi, ewj = wj;
    asm volatile("" : "+v"(elm), "+v"(elk), "+s"(ewi), "+s"(ewj));
    const unsigned lane_off = (unsigned)(elk * n + elm);
    double *const tile_d = sim + i0 * n + j0, *const tile_m = sim + j0 * n + i0;
    const long long rem_i = n - i0 - ewi, rem_j = n - j0 - ewj;       // valid rows / columns from the wave's block origin
#pragma unroll
    for (int b = 0; b < 4; ++b) {
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            __builtin_amdgcn_sched_barrier(0);
            const double ccb = nrm[128 + ewj + 16 * b + elm];
            const bool on_diag_tile = !mirror;
            double v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double cosv = acc[a][b][r] * (nrm[ewi + 16 * a + elk + 4 * r] * ccb);
                if (fabs(cosv) > 1.0) cosv = copysign(1.0, cosv);
                const double dist = 1.0 - cosv;
                v[r] = (on_diag_tile && ewi + 16 * a + 4 * r + elk == ewj + 16 * b + elm) ? 1.0 : 1.0 - dist;
                if (16 * a + 4 * r + elk < rem_i && 16 * b + elm < rem_j)
                    (tile_d + ((long long)(ewi + 16 * a + 4 * r) * n + ewj + 16 * b))[lane_off] = v[r];
            }
            if (mirror) {
#pragma unroll
                for (int r = 0; r < 4; ++r) tr[(elk + 4 * r) * 17 + elm] = v[r];
                wsync();
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double w = tr[elm * 17 + elk + 4 * r];
                    if (16 * b + 4 * r + elk < rem_j && 16 * a + elm < rem_i)
                        (tile_m + ((long long)(ewj + 16 * b + 4 * r) * n + ewi + 16 * a))[lane_off] = w;
                }
                wsync();
            }
        }
    }
    if (tile + gridDim.x < n_tiles) {             // first chunk of this workgroup's next tile
        PAA_SIMB_TILE(tile + gridDim.x)
        PAA_SIMB_FETCH(0, ti * kSimTile, tj * kSimTile)
    }
    }   // tile loop
#undef PAA_SIMB_FETCH
#undef PAA_SIMB_TILE
}

// one block per list entry (clip, bx, by): thumb_diag_kernel's block (bx, by) of that clip
__global__ __launch_bounds__(256) void thumb_diag_batch_kernel(const double *__restrict__ simbuf,
                                                                const ThumbClip *__restrict__ clips,
                                                                const ThumbBlock *__restrict__ blocks, int M, double band,
                                                                double *__restrict__ filtbuf, double *__restrict__ cand) {
    __shared__ double red[4];
    __shared__ double rv[4];
    __shared__ long long ri[4];
    const ThumbBlock tb = blocks[blockIdx.x];
    const ThumbClip c = clips[tb.clip];
    const double *sim = simbuf + c.sim_off;
    double *out = filtbuf + c.filt_off;
    const long long n = c.n, R = c.R, lim_lo = c.lim_lo, lim_hi = c.lim_hi;
    const long long i0 = (long long)tb.by * kDiagRun;
    const long long d = (long long)tb.bx * 256 + threadIdx.x;
    double vmin = __builtin_inf();
    double v = -__builtin_inf();
    long long vi = 0x7fffffffffffffffLL;
    const long long lim = R - i0 - d;                               // cells of this diagonal run inside the matrix
    const int cnt = lim < kDiagRun ? (int)lim : kDiagRun;
    if (cnt > 0) {
        const long long dstep = n + 1, ostep = R + 1;
        const double *p = sim + i0 * n + (i0 + d);                  // S[i][j] of the first cell
        double run = 0.0;
        for (int k = 0; k < M; ++k) run += p[k * dstep];
        double *o = out + i0 * R + (i0 + d);
        const bool diag_masked = fabs((double)d) < band;
        const long long idx0 = i0 * R + (i0 + d);
        const long long lo_ = lim_lo - i0, hi_ = lim_hi - d - i0;       // s range of the unmasked cells
        const int s_lo = lo_ < 0 ? 0 : (lo_ > kDiagRun ? kDiagRun : (int)lo_), s_hi = hi_ < 0 ? 0 : (hi_ > kDiagRun ? kDiagRun : (int)hi_);
        const double *pn = p + (long long)M * dstep;
#pragma unroll 8
        for (int s = 0; s < cnt; ++s) {
            if (s > 0) {
                const double gone = p[(s - 1) * dstep];
                if (gone != gone) {
                    run = 0.0;
                    for (int k = 0; k < M; ++k) run += p[(s + k) * dstep];
                } else {
                    run += pn[(s - 1) * dstep] - gone;
                }
            }
            vmin = nan_min(vmin, run);
            if (!diag_masked && s >= s_lo && s < s_hi) {
                o[s * ostep] = run;
                if (argmax_better(run, idx0 + s * ostep, v, vi)) { v = run; vi = idx0 + s * ostep; }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        vmin = nan_min(vmin, __shfl_xor(vmin, off, 64));
        const double ov = __shfl_xor(v, off, 64);
        const long long oi = __shfl_xor(vi, off, 64);
        if (argmax_better(ov, oi, v, vi)) { v = ov; vi = oi; }
    }
    if (lane == 0) { red[wave] = vmin; rv[wave] = v; ri[wave] = vi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            vmin = nan_min(vmin, red[w]);
            if (argmax_better(rv[w], ri[w], v, vi)) { v = rv[w]; vi = ri[w]; }
        }
        const long long n_blk = (long long)c.gx * c.gy, blk = (long long)tb.by * c.gx + tb.bx;
        double *block_min = cand + c.cand_off, *cand_val = block_min + n_blk + 1;
        long long *cand_idx = reinterpret_cast<long long *>(cand_val + n_blk);
        block_min[blk] = vmin;
        cand_val[blk] = v;
        cand_idx[blk] = vi;
    }
}

// one workgroup per clip: thumb_min_kernel over the clip's slots
__global__ __launch_bounds__(1024) void thumb_min_batch_kernel(const ThumbClip *__restrict__ clips, double *__restrict__ cand) {
    __shared__ double red[16];
    const ThumbClip c = clips[blockIdx.x];
    const long long n_blk = (long long)c.gx * c.gy;
    double *block_min = cand + c.cand_off;
    double m = __builtin_inf();
    for (long long b = threadIdx.x; b < n_blk; b += 1024)
        m = nan_min(m, diag_block_live(b % c.gx, b / c.gx, c.R) ? block_min[b] : __builtin_inf());
    for (int off = 1; off < 64; off <<= 1) m = nan_min(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) m = nan_min(m, red[w]);
        block_min[n_blk] = m;
    }
}

// grid (list of (clip, row block by), column block): thumb_fill_kernel's block (blockIdx.y, by) of that clip
__global__ __launch_bounds__(256) void thumb_fill_batch_kernel(const ThumbClip *__restrict__ clips,
                                                                const ThumbBlock *__restrict__ rows, double band,
                                                                double *__restrict__ filtbuf, const double *__restrict__ cand) {
    const ThumbBlock tb = rows[blockIdx.x];
    const ThumbClip c = clips[tb.clip];
    const long long R = c.R;
    if ((long long)blockIdx.y * 1024 >= R) return;
    double *f = filtbuf + c.filt_off;
    const double min_sm = cand[c.cand_off + (long long)c.gx * c.gy];
    for (int rr = 0; rr < kMaskRows; ++rr) {
        const long long i = (long long)tb.by * kMaskRows + rr;
        if (i >= R) break;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long j = (long long)blockIdx.y * 1024 + 256 * q + threadIdx.x;
            if (j < R && thumb_masked(i, j, band, c.lim_lo, c.lim_hi)) f[i * R + j] = min_sm;
        }
    }
}

// one workgroup per clip: thumb_argmax_kernel over the clip's slots, degenerate path and NaN rule included; pos [n][2]
__global__ __launch_bounds__(1024) void thumb_argmax_batch_kernel(const ThumbClip *__restrict__ clips, double band,
                                                                   double *__restrict__ cand, long long *__restrict__ pos) {
    __shared__ double rv[16];
    __shared__ long long ri[16];
    const ThumbClip c = clips[blockIdx.x];
    const long long n_blk = (long long)c.gx * c.gy, R = c.R, lim_lo = c.lim_lo, lim_hi = c.lim_hi;
    const double *block_min = cand + c.cand_off, *cand_val = block_min + n_blk + 1;
    const long long *cand_idx = reinterpret_cast<const long long *>(cand_val + n_blk);
    double v = -__builtin_inf();
    long long vi = 0x7fffffffffffffffLL;
    for (long long b = threadIdx.x; b < n_blk; b += 1024) {
        const bool live = diag_block_live(b % c.gx, b / c.gx, R);
        const double ov = live ? cand_val[b] : -__builtin_inf();
        const long long oi = live ? cand_idx[b] : 0x7fffffffffffffffLL;
        if (argmax_better(ov, oi, v, vi)) { v = ov; vi = oi; }
    }
    for (int off = 1; off < 64; off <<= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const long long oi = __shfl_xor(vi, off, 64);
        if (argmax_better(ov, oi, v, vi)) { v = ov; vi = oi; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { rv[wave] = v; ri[wave] = vi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w)
            if (argmax_better(rv[w], ri[w], v, vi)) { v = rv[w]; vi = ri[w]; }
        const double m = block_min[n_blk];
        const bool m_nan = m != m;
        const bool unmasked_wins = (vi != 0x7fffffffffffffffLL) && !m_nan && v > m;
        if (!unmasked_wins) {
            long long first_masked = 0x7fffffffffffffffLL;
            for (long long i = 0; i < R && first_masked == 0x7fffffffffffffffLL; ++i) {
                if (thumb_masked(i, 0, band, lim_lo, lim_hi)) first_masked = i * R;
                else if (lim_hi < R) first_masked = i * R + (lim_hi > 0 ? lim_hi : 0);     // columns >= lim_hi are masked
            }
            const bool tie = (vi != 0x7fffffffffffffffLL) && (m_nan ? (v != v) : (v == m));
            vi = (tie && vi < first_masked) ? vi : first_masked;
        }
        reinterpret_cast<long long *>(cand)[c.cand_off + 3 * n_blk + 1] = vi;
        pos[2 * (long long)blockIdx.x] = vi / R;
        pos[2 * (long long)blockIdx.x + 1] = vi % R;
    }
}

// thread per clip: the arg-max cell grows along its diagonal until it spans M cells (audioSegmentation.py:1167-1182, the
// comparisons and the four break conditions of audioSegmentation._grow_thumbnail; `>` is false on NaN: a NaN grows forward).
// bounds [n][4] = (i1, i2, j1, j2)
__global__ __launch_bounds__(64) void thumb_grow_batch_kernel(const ThumbClip *__restrict__ clips, long long n_clips, int M,
                                                               const double *__restrict__ filtbuf,
                                                               const long long *__restrict__ pos,
                                                               long long *__restrict__ bounds) {
    const long long k = (long long)blockIdx.x * 64 + threadIdx.x;
    if (k >= n_clips) return;
    const long long R = clips[k].R, last = R - 2;
    const double *f = filtbuf + clips[k].filt_off;
    long long i1 = pos[2 * k], i2 = i1, j1 = pos[2 * k + 1], j2 = j1;
    while (i2 - i1 < M) {
        if (i1 <= 0 || j1 <= 0 || i2 >= last || j2 >= last) break;
        if (f[(i1 - 1) * R + (j1 - 1)] > f[(i2 + 1) * R + (j2 + 1)]) { --i1; --j1; }
        else { ++i2; ++j2; }
    }
    bounds[4 * k] = i1;
    bounds[4 * k + 1] = i2;
    bounds[4 * k + 2] = j1;
    bounds[4 * k + 3] = j2;
}

}  // namespace simb
}  // namespace paa
