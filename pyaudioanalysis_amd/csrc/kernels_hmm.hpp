// Gaussian hidden Markov models with diagonal "covariances" for joint segmentation-classification: what
// audioSegmentation.hmm_segmentation asks of hmmlearn's GaussianHMM.predict (audioSegmentation.py:470-492) and
// train_hmm_compute_statistics (:287-344) computes in NumPy.  All FP64.
//
//  * emission_kernel: B[t][k] = -0.5 (D log 2 pi + sum_d log c[k][d] + sum_d (x[t][d] - mu[k][d])^2 / c[k][d]) from the
//    feature-major matrix feats [n_dims][ld]: one lane per window t (coalesced reads, the matrix is read once), the K sums
//    in registers, mu and 1 / c read through wave-uniform (scalar) loads from the [d][KP] tables.  c is what the reference
//    stores in covars_: the per-class standard deviation (:340).
//  * Viterbi with hmmlearn's semantics (lowest index among equal maxima everywhere).  A GROUP of KP lanes (KP = K rounded
//    up to a power of two, at least 2; padded states have log-probability -inf everywhere) owns one recursion, lane j the
//    state j: lat'[j] = max_i(lat[i] + logA[i][j]) + B[t][j] with lat[i] fetched by a group shuffle and column j of logA in
//    registers; 64 / KP recursions share a wave.  Only additions of -inf occur (never inf - inf), so no NaN arises.
//    Every sequence is cut into SEGMENTS of at most `block_rows` rows:
//      (A) product_kernel:  for a segment that is not its sequence's last and every entering state i, the recursion from
//          the unit vector e_i: row i of the segment's (max,+) product M[i][j];
//      (B) chain_kernel:    per sequence, serially over its segments, v <- max_i(v[i] + M[i][j]): the lattice vector
//          entering each segment;
//      (C) segment_kernel:  per segment, the plain recursion from its entering vector with the back-pointers
//          psi[t][j] = argmax_i(lat[t-1][i] + logA[i][j]) (the expression hmmlearn re-evaluates when it backtracks), then
//          every lane j walks the pointers back from END state j and leaves P[t][j], the state at t on that path, in place
//          of psi, and the state the path enters the segment from (a K -> K map);
//      (D) pick_kernel:     per sequence, the last state and log-probability and the serial composition of the maps;
//      (E) gather_kernel:   states[t] = P[t][end state of t's segment].
//    A sequence of at most block_rows rows is one segment and skips (A) and (B).
//  * stats kernels: class counts and transition counts (integer atomics), per-class mean and population standard
//    deviation of every feature row, two-pass about the mean as np.std does.
#pragma once
#include "device_common.hpp"
#include "model_launch.hpp"

namespace paa {
namespace hmm {

constexpr int kEmitThreads = 64;
constexpr int kChunk = 256;           // rows of back-pointers staged in LDS per group and step of the walk back
constexpr int kStatThreads = 256;

template <int KP>
__global__ __launch_bounds__(kEmitThreads) void emission_kernel(HmmDev m, const double *__restrict__ feats, long long ld,
                                                                long long n_vec, double *__restrict__ B) {
    const long long t = (long long)blockIdx.x * kEmitThreads + threadIdx.x;
    const bool live = t < n_vec;
    const double *x = feats + (live ? t : n_vec - 1);
    double acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.0;
    constexpr int U = 8;
    int d = 0;
    for (; d + U <= m.n_dims; d += U) {
        double xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = x[(long long)(d + u) * ld];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                const double df = xv[u] - m.mu[(d + u) * KP + k];
                acc[k] = fma(df * df, m.inv[(d + u) * KP + k], acc[k]);
            }
        }
    }
    for (; d < m.n_dims; ++d) {
        const double xv = x[(long long)d * ld];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const double df = xv - m.mu[d * KP + k];
            acc[k] = fma(df * df, m.inv[d * KP + k], acc[k]);
        }
    }
    if (!live) return;
#pragma unroll
    for (int k = 0; k < KP; ++k)
        if (k < m.n_states) B[t * m.n_states + k] = -0.5 * (m.cst[k] + acc[k]);
}

// one step of the recursion for lane j of a group: a[i] = logA[i][j]; the first maximum wins
template <int KP>
__device__ __forceinline__ void viterbi_step(double &lat, int &arg, const double (&a)[KP], double b) {
    double best = __shfl(lat, 0, KP) + a[0];
    int bi = 0;
#pragma unroll
    for (int i = 1; i < KP; ++i) {
        const double c = __shfl(lat, i, KP) + a[i];
        if (c > best) { best = c; bi = i; }
    }
    lat = best + b;
    arg = bi;
}

// rows t0 .. t1 - 1 of the recursion (group-uniform bounds); B rows are fetched eight steps ahead
template <int KP, bool PSI>
__device__ __forceinline__ void viterbi_forward(const HmmDev &m, const double (&a)[KP], double &lat, const double *B,
                                                long long t0, long long t1, int j, unsigned char *psi) {
    constexpr int U = 8;
    const int K = m.n_states;
    const bool act = j < K;
    const double ninf = -__builtin_inf();
    double bc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) bc[u] = (act && t0 + u < t1) ? B[(t0 + u) * K + j] : ninf;
    for (long long t = t0; t < t1; t += U) {
        double bn[U];
#pragma unroll
        for (int u = 0; u < U; ++u) bn[u] = (act && t + U + u < t1) ? B[(t + U + u) * K + j] : ninf;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (t + u < t1) {
                int arg;
                viterbi_step<KP>(lat, arg, a, bc[u]);
                if (PSI) psi[(t + u) * KP + j] = (unsigned char)arg;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) bc[u] = bn[u];
    }
}

template <int KP>
__device__ __forceinline__ void load_column(const HmmDev &m, int j, double (&a)[KP]) {
#pragma unroll
    for (int i = 0; i < KP; ++i) a[i] = m.logA[i * KP + j];
}

// (A) group (segment s, entering state i): M[s][i][j]
template <int KP>
__global__ __launch_bounds__(64) void product_kernel(HmmDev m, const double *__restrict__ B, const Segment *__restrict__ segs,
                                                     long long n_seg, double *__restrict__ M) {
    constexpr int G = 64 / KP;
    const int j = threadIdx.x % KP;
    const long long task = (long long)blockIdx.x * G + threadIdx.x / KP;
    if (task >= n_seg * m.n_states) return;
    const long long s = task / m.n_states;
    const int i = (int)(task % m.n_states);
    const Segment sg = segs[s];
    if (sg.last) return;
    double a[KP];
    load_column<KP>(m, j, a);
    double lat = j == i ? 0.0 : -__builtin_inf();
    viterbi_forward<KP, false>(m, a, lat, B, sg.first ? sg.r0 + 1 : sg.r0, sg.r1, j, nullptr);
    M[(s * KP + i) * KP + j] = lat;
}

// (B) group per sequence: V[s] = the lattice vector entering segment s (not written for a sequence's first segment)
template <int KP>
__global__ __launch_bounds__(64) void chain_kernel(HmmDev m, const double *__restrict__ B, const Segment *__restrict__ segs,
                                                   const long long *__restrict__ seq_seg, long long n_seq,
                                                   const double *__restrict__ M, double *__restrict__ V) {
    constexpr int G = 64 / KP;
    const int j = threadIdx.x % KP;
    const long long q = (long long)blockIdx.x * G + threadIdx.x / KP;
    if (q >= n_seq) return;
    const long long s0 = seq_seg[q], s1 = seq_seg[q + 1];
    if (s1 - s0 < 2) return;
    double lat = m.logpi[j] + (j < m.n_states ? B[segs[s0].r0 * m.n_states + j] : -__builtin_inf());
    double mc[KP], mn[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) { mc[i] = M[(s0 * KP + i) * KP + j]; mn[i] = 0.0; }
    for (long long s = s0; s + 1 < s1; ++s) {
        if (s + 2 < s1) {
#pragma unroll
            for (int i = 0; i < KP; ++i) mn[i] = M[((s + 1) * KP + i) * KP + j];
        }
        int arg;
        viterbi_step<KP>(lat, arg, mc, 0.0);
        V[(s + 1) * KP + j] = lat;
#pragma unroll
        for (int i = 0; i < KP; ++i) mc[i] = mn[i];
    }
}

// (C) group per segment
template <int KP>
__global__ __launch_bounds__(64) void segment_kernel(HmmDev m, const double *__restrict__ B, const Segment *__restrict__ segs,
                                                     long long n_seg, const double *__restrict__ V, double *__restrict__ Vout,
                                                     unsigned char *psi, unsigned char *__restrict__ emap) {
    __shared__ unsigned char staged[64 * kChunk];      // [group][kChunk][KP]
    const int j = threadIdx.x % KP, g = threadIdx.x / KP;
    const long long s = (long long)blockIdx.x * (64 / KP) + g;
    if (s >= n_seg) return;
    const Segment sg = segs[s];
    double a[KP];
    load_column<KP>(m, j, a);
    double lat;
    long long start;
    if (sg.first) {
        lat = m.logpi[j] + (j < m.n_states ? B[sg.r0 * m.n_states + j] : -__builtin_inf());
        start = sg.r0 + 1;
    } else {
        lat = V[s * KP + j];
        start = sg.r0;
    }
    viterbi_forward<KP, true>(m, a, lat, B, start, sg.r1, j, psi);
    Vout[s * KP + j] = lat;
    // walk back from every end state j at once; a lane stages the pointers it wrote itself
    unsigned char *mine = staged + g * (kChunk * KP);
    int cur = j;
    for (long long c1 = sg.r1; c1 > start; c1 -= kChunk) {
        const long long c0 = c1 - kChunk > start ? c1 - kChunk : start;
        const int n = (int)(c1 - c0);
        constexpr int U = 16;
        for (int u = 0; u < n; u += U) {
            unsigned char r[U];
#pragma unroll
            for (int v = 0; v < U; ++v) r[v] = u + v < n ? psi[(c0 + u + v) * KP + j] : (unsigned char)0;
#pragma unroll
            for (int v = 0; v < U; ++v)
                if (u + v < n) mine[(u + v) * KP + j] = r[v];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (int u = n - 1; u >= 0; --u) {
            psi[(c0 + u) * KP + j] = (unsigned char)cur;
            cur = mine[u * KP + cur];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    if (sg.first) psi[sg.r0 * KP + j] = (unsigned char)cur;
    else emap[s * KP + j] = (unsigned char)cur;
}

// (D) one workgroup of 64 lanes per sequence: logprob, and the end state of every segment into seg_end
__global__ __launch_bounds__(64) void pick_kernel(int n_states, int kp, const long long *__restrict__ seq_seg,
                                                  const double *__restrict__ Vout, const unsigned char *__restrict__ emap,
                                                  int *__restrict__ seg_end, double *__restrict__ logprob) {
    __shared__ unsigned char maps[64 * kMaxStates];
    __shared__ int carry;
    const long long q = blockIdx.x;
    const long long s0 = seq_seg[q], s1 = seq_seg[q + 1];
    const int lane = threadIdx.x;
    if (lane == 0) {
        const double *v = Vout + (s1 - 1) * kp;
        int e = 0;
        double best = v[0];
        for (int k = 1; k < n_states; ++k)
            if (v[k] > best) { best = v[k]; e = k; }
        logprob[q] = best;
        seg_end[s1 - 1] = e;
        carry = e;
    }
    // segments hi - 1 .. lo (chunks of 64, from the back): seg_end[s - 1] = emap[s][seg_end[s]]
    for (long long hi = s1; hi > s0 + 1; hi -= 64) {
        const long long lo = hi - 64 > s0 + 1 ? hi - 64 : s0 + 1;
        __syncthreads();
        if (lo + lane < hi)
            for (int k = 0; k < kp; ++k) maps[lane * kp + k] = emap[(lo + lane) * kp + k];
        __syncthreads();
        if (lane == 0) {
            int e = carry;
            for (long long s = hi - 1; s >= lo; --s) {
                e = maps[(s - lo) * kp + e];
                seg_end[s - 1] = e;
            }
            carry = e;
        }
    }
}

// (E) one workgroup per segment
__global__ __launch_bounds__(64) void gather_kernel(int kp, const Segment *__restrict__ segs, const int *__restrict__ seg_end,
                                                    const unsigned char *__restrict__ P, int *__restrict__ states) {
    const Segment sg = segs[blockIdx.x];
    const int e = seg_end[blockIdx.x];
    for (long long t = sg.r0 + threadIdx.x; t < sg.r1; t += 64) states[t] = P[t * kp + e];
}

// counts[k] and counts[K + a K + b] (transitions a -> b of consecutive labels); `counts` is zero on entry
__global__ __launch_bounds__(kStatThreads) void stats_count_kernel(const int *__restrict__ labels, long long n, int K,
                                                                   int *__restrict__ counts) {
    __shared__ int local[kMaxStates + kMaxStates * kMaxStates];
    const int cells = K + K * K;
    for (int i = threadIdx.x; i < cells; i += kStatThreads) local[i] = 0;
    __syncthreads();
    for (long long t = (long long)blockIdx.x * kStatThreads + threadIdx.x; t < n; t += (long long)gridDim.x * kStatThreads) {
        const int a = labels[t];
        atomicAdd(&local[a], 1);
        if (t + 1 < n) atomicAdd(&local[K + a * K + labels[t + 1]], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += kStatThreads)
        if (local[i]) atomicAdd(&counts[i], local[i]);
}

__device__ __forceinline__ double stats_block_sum(double v, double *red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = kStatThreads / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

// workgroup (feature row d, class k): mean and population standard deviation over the windows labelled k
__global__ __launch_bounds__(kStatThreads) void stats_moment_kernel(const double *__restrict__ feats, long long ld, long long n,
                                                                    const int *__restrict__ labels, int K,
                                                                    const int *__restrict__ counts, double *__restrict__ means,
                                                                    double *__restrict__ stds, int n_dims) {
    __shared__ double red[kStatThreads];
    const int k = blockIdx.x % K, d = blockIdx.x / K;
    const double *x = feats + (long long)d * ld;
    const double cnt = (double)counts[k];
    double s = 0.0;
    for (long long t = threadIdx.x; t < n; t += kStatThreads)
        if (labels[t] == k) s += x[t];
    const double mean = stats_block_sum(s, red) / cnt;
    double ss = 0.0;
    for (long long t = threadIdx.x; t < n; t += kStatThreads)
        if (labels[t] == k) { const double df = x[t] - mean; ss = fma(df, df, ss); }
    const double var = stats_block_sum(ss, red) / cnt;
    if (threadIdx.x == 0) {
        means[(long long)k * n_dims + d] = mean;
        stds[(long long)k * n_dims + d] = sqrt(var);
    }
}

}  // namespace hmm
}  // namespace paa
