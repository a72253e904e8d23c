// The glue of audioSegmentation.silence_removal around its SVM fit, for a batch of clips whose short-term matrices [n_dims][T]
// stay in HBM (audioSegmentation.py:713-761): the energy limits and the quiet / loud frames (onset_select_kernel), the training
// matrix and its scaler (onset_gather_kernel), the fit folded into one weight vector per clip (onset_weights_kernel), the onset
// probability of every frame of every clip (onset_proba_kernel, the bank form of svm_binary_proba_kernel) and smoothing,
// threshold and activity flags (onset_threshold_kernel).
//
// One workgroup per clip wherever an order matters.  The reference sorts the energies (and later the smoothed probabilities)
// only to average their lowest and highest tenth; here the value of the rank that bounds a tenth comes from a radix select
// over the order-preserving 64-bit keys of the doubles (eight passes of eight bits, an LDS histogram of integer counts each),
// and the mean from one more pass: the values strictly beyond that value are added, the ties at it are counted.  No pass keeps
// more than a histogram in LDS, so a clip may have any number of frames.  Every sum is formed in a fixed order -- a thread adds
// its frames tid, tid + 256, ... in that order, the workgroup adds the 256 partial sums in a fixed tree -- and nothing is added
// atomically: a clip's numbers are the same bits alone and anywhere in a batch.
#pragma once
#include "kernels_svm_prob.hpp"
#include "model_launch.hpp"

namespace paa {
namespace onset {

// v < w  <=>  order_key(v) < order_key(w) for doubles that are not NaN (-0.0 sorts below +0.0)
__device__ __forceinline__ unsigned long long order_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// the workgroup's sum of x in a fixed tree; red [kThreads] in LDS.  Every thread returns the same value
template <typename T>
__device__ __forceinline__ T block_sum(T x, T *red, int tid) {
    __syncthreads();                                    // the previous use of red is over
    red[tid] = x;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// The value of rank k (0-based, ascending) among v[0 .. n - 1], 0 <= k < n; hist [256] and pick [2] in LDS.  Every thread
// returns the same value
__device__ __forceinline__ double block_select(const double *__restrict__ v, int n, int k, int *hist, int *pick, int tid) {
    unsigned long long prefix = 0, mask = 0;
    int rank = k;
    for (int shift = 56; shift >= 0; shift -= 8) {
        __syncthreads();                                // the previous use of hist and pick is over
        hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += kThreads) {
            const unsigned long long key = order_key(v[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int below = 0, b = 0;
            for (; b < 255; ++b) {
                if (rank < below + hist[b]) break;
                below += hist[b];
            }
            pick[0] = b;
            pick[1] = rank - below;
        }
        __syncthreads();
        prefix |= (unsigned long long)pick[0] << shift;
        mask |= 255ull << shift;
        rank = pick[1];
    }
    return key_value(prefix);
}

// Stage 1.  Workgroup c: tenth = T / 10 (the host admits T >= 20 only);
//   quiet_limit = mean of the tenth smallest energies + 1e-15,
//   loud_limit  = mean of the tenth largest without one instance of the maximum (ranked[-tenth:-1]) + 1e-15,
// limits [n_clips][2]; the flags energy <= quiet_limit and energy >= loud_limit of every frame; counts [n_clips][2]
__global__ __launch_bounds__(kThreads) void onset_select_kernel(OnsetDev m) {
    __shared__ int hist[kThreads], pick[2];
    __shared__ double red[kThreads];
    int *ired = hist;                                   // (block_sum<int> never overlaps a select)
    const int tid = threadIdx.x;
    const ClipRec C = m.clips[blockIdx.x];
    const int T = C.T, tenth = T / 10;
    const double *__restrict__ e = m.feats + C.feat_off + (long long)T;      // row 1: the energy
    if (tenth < 2) {                                    // no limits exist: nothing is flagged
        for (int t = tid; t < T; t += kThreads) { m.quiet[C.frame_off + t] = 0; m.loud[C.frame_off + t] = 0; }
        if (tid == 0) {
            m.limits[2 * blockIdx.x] = m.limits[2 * blockIdx.x + 1] = 0.0;
            m.counts[2 * blockIdx.x] = m.counts[2 * blockIdx.x + 1] = 0;
        }
        return;
    }
    const double v_lo = block_select(e, T, tenth - 1, hist, pick, tid);
    const double v_hi = block_select(e, T, T - tenth, hist, pick, tid);
    const double v_max = block_select(e, T, T - 1, hist, pick, tid);
    double s_lo = 0.0, s_mid = 0.0;
    int c_lo = 0, c_gt = 0, c_max = 0;
    for (int t = tid; t < T; t += kThreads) {
        const double x = e[t];
        if (x < v_lo) { s_lo += x; ++c_lo; }
        if (x > v_hi) {
            ++c_gt;
            if (x < v_max) s_mid += x;
            else ++c_max;
        }
    }
    s_lo = block_sum(s_lo, red, tid);
    s_mid = block_sum(s_mid, red, tid);
    c_lo = block_sum(c_lo, ired, tid);
    c_gt = block_sum(c_gt, ired, tid);
    c_max = block_sum(c_max, ired, tid);
    const double low = s_lo + (double)(tenth - c_lo) * v_lo;
    const double high = v_max > v_hi ? s_mid + (double)(c_max - 1) * v_max + (double)(tenth - c_gt) * v_hi : (double)(tenth - 1) * v_hi;
    const double quiet_limit = low / (double)tenth + 1e-15, loud_limit = high / (double)(tenth - 1) + 1e-15;
    int n_quiet = 0, n_loud = 0;
    for (int t = tid; t < T; t += kThreads) {
        const double x = e[t];
        const bool q = x <= quiet_limit, l = x >= loud_limit;
        m.quiet[C.frame_off + t] = q;
        m.loud[C.frame_off + t] = l;
        n_quiet += q;
        n_loud += l;
    }
    n_quiet = block_sum(n_quiet, ired, tid);
    n_loud = block_sum(n_loud, ired, tid);
    if (tid == 0) {
        m.limits[2 * blockIdx.x] = quiet_limit;
        m.limits[2 * blockIdx.x + 1] = loud_limit;
        m.counts[2 * blockIdx.x] = n_quiet;
        m.counts[2 * blockIdx.x + 1] = n_loud;
    }
}

// the frames t of the clip with flag[t] set, in frame order, to list[0 .. cap - 1]; wave_n [kThreads / 64] in LDS
__device__ __forceinline__ void compact_frames(const unsigned char *__restrict__ flag, int T, int *list, int cap, int *wave_n, int tid) {
    const int lane = tid % 64, wave = tid / 64;
    int base = 0;
    for (int t0 = 0; t0 < T; t0 += kThreads) {
        const int t = t0 + tid;
        const bool f = t < T && flag[t] != 0;
        const unsigned long long ballot = __ballot(f);
        __syncthreads();                                // the previous use of wave_n is over
        if (lane == 0) wave_n[wave] = __popcll(ballot);
        __syncthreads();
        int before = base, all = 0;
        for (int w = 0; w < kThreads / 64; ++w) {
            if (w < wave) before += wave_n[w];
            all += wave_n[w];
        }
        const int pos = before + __popcll(ballot & ((1ull << lane) - 1ull));
        if (f && pos < cap) list[pos] = t;
        base += all;
    }
}

// Stage 2.  Workgroup c, from the flags of stage 1 and the counts the host read (ClipRec n_quiet, n_loud, row_off): src
// [row_off ..] = the quiet frames in frame order, then the loud frames in frame order; X [row_off + r][n_dims] = frame src[r],
// sample-major; mean [c][n_dims] = the column sums in row order / n; scale = sqrt(sum of (x - mean)^2 in row order / n), 1 where
// it is below 10 eps.  Plain sequential adds without contraction: NumPy's axis-0 reductions, bit for bit.
// A deliberate trade: the copy reads frames T doubles apart (its writes are the coalesced side) and pays a 64-bit divide per
// element, and the scaler is n_dims threads walking the rows one after the other while the rest of the workgroup idles -- a tree
// or a split over rows would change the summation order and lose NumPy's bits.  Measured: 0.16 ms for 200 clips of about 110
// rows, 0.35 ms for 50 clips of about 1000 (profiles/bench_silence_batch_n1_local.json)
#pragma clang fp contract(off)
__global__ __launch_bounds__(kThreads) void onset_gather_kernel(OnsetDev m) {
    __shared__ int wave_n[kThreads / 64];
    const int tid = threadIdx.x;
    const ClipRec C = m.clips[blockIdx.x];
    const int T = C.T, D = m.n_dims;
    const long long n = (long long)C.n_quiet + C.n_loud;
    const double *__restrict__ f = m.feats + C.feat_off;
    int *src = m.src + C.row_off;
    compact_frames(m.quiet + C.frame_off, T, src, C.n_quiet, wave_n, tid);
    compact_frames(m.loud + C.frame_off, T, src + C.n_quiet, C.n_loud, wave_n, tid);
    __syncthreads();                                    // src is complete
    double *X = m.X + C.row_off * D;
    for (long long i = tid; i < n * D; i += kThreads) {
        const long long r = i / D;
        const int d = (int)(i - r * D);
        X[i] = f[(long long)d * T + src[r]];
    }
    __syncthreads();                                    // X is complete
    if (tid >= D) return;
    double mean = 0.0, scale = 1.0;
    if (n > 0) {
        const double *__restrict__ x = X + tid;
        double s = 0.0;
        long long r = 0;
        for (; r + 4 <= n; r += 4) {
            const double a0 = x[r * D], a1 = x[(r + 1) * D], a2 = x[(r + 2) * D], a3 = x[(r + 3) * D];
            s += a0; s += a1; s += a2; s += a3;
        }
        for (; r < n; ++r) s += x[r * D];
        mean = s / (double)n;
        s = 0.0;
        for (r = 0; r + 4 <= n; r += 4) {
            const double d0 = x[r * D] - mean, d1 = x[(r + 1) * D] - mean, d2 = x[(r + 2) * D] - mean, d3 = x[(r + 3) * D] - mean;
            s += d0 * d0; s += d1 * d1; s += d2 * d2; s += d3 * d3;
        }
        for (; r < n; ++r) { const double d0 = x[r * D] - mean; s += d0 * d0; }
        scale = sqrt(s / (double)n);
        if (scale < 10.0 * 2.220446049250313e-16) scale = 1.0;
    }
    m.mean[(long long)blockIdx.x * D + tid] = mean;
    m.scale[(long long)blockIdx.x * D + tid] = scale;
}

// Between stages 3 and 4.  Workgroup c folds its fit into scikit-learn's linear model: w [c][n_dims] = the sum over its rows
// with alpha_y != 0, in row order, of -alpha_y (x - mean) / scale (dual_coef_ times the standardised support vector, product
// rounded, then added); intercept [c] = rho
__global__ __launch_bounds__(kThreads) void onset_weights_kernel(OnsetDev m) {
    const int tid = threadIdx.x, D = m.n_dims;
    const ClipRec C = m.clips[blockIdx.x];
    const long long n = (long long)C.n_quiet + C.n_loud;
    if (tid == 0) m.intercept[blockIdx.x] = m.rho[blockIdx.x];
    if (tid >= D) return;
    const double *__restrict__ x = m.X + C.row_off * D + tid;
    const double *__restrict__ ay = m.alpha_y + C.row_off;
    const double mean = m.mean[(long long)blockIdx.x * D + tid], scale = m.scale[(long long)blockIdx.x * D + tid];
    double w = 0.0;
    for (long long r = 0; r < n; ++r) {
        const double a = ay[r];
        if (a == 0.0) continue;                         // not a support vector (the same for the whole workgroup)
        const double z = (x[r * D] - mean) / scale;
        w += -a * z;
    }
    m.w[(long long)blockIdx.x * D + tid] = w;
}
#pragma clang fp contract(fast)

// Stage 4.  One thread per frame of the batch: frame g belongs to the clip c with frame_off[c] <= g < frame_off[c + 1] and is
// scored as svm_binary_proba_kernel scores it with the one "support vector" w [c] of coefficient 1: standardise with mean [c]
// / scale [c], dec = <w, z> + intercept, the Platt sigmoid with A [c] / B [c], the clamp and libsvm's two-class coupling
__global__ __launch_bounds__(kThreads) void onset_proba_kernel(OnsetDev m, int n_clips, long long n_frames) {
    const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (g >= n_frames) return;
    int lo = 0, hi = n_clips - 1;                       // the last clip with frame_off <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (m.clips[mid].frame_off <= g) lo = mid;
        else hi = mid - 1;
    }
    const ClipRec C = m.clips[lo];
    const int D = m.n_dims;
    const long long t = g - C.frame_off;
    if (t >= C.T) return;
    const double *__restrict__ f = m.feats + C.feat_off + t;
    const double *__restrict__ mean = m.mean + (long long)lo * D;
    const double *__restrict__ scale = m.scale + (long long)lo * D;
    const double *__restrict__ w = m.w + (long long)lo * D;
    double k = 0.0;
    for (int d = 0; d < D; ++d) k = fma(w[d], (f[(long long)d * C.T] - mean[d]) / scale[d], k);
    const double dec = k + m.intercept[lo];             // = sklearn's decision_function; libsvm's own decision value is -dec
    const double fApB = (-dec) * m.A[lo] + m.B[lo];
    double p = (fApB >= 0.0) ? exp(-fApB) / (1.0 + exp(-fApB)) : 1.0 / (1.0 + exp(fApB));
    p = fmin(fmax(p, 1e-7), 1.0 - 1e-7);
    m.raw[g] = libsvm_two_class_prob1(p);
}

// Stage 5.  Workgroup c: prob = smooth_moving_avg(raw, width) (the ends continued by point reflection about the first / last
// value, out[i] the mean of the `width` entries of the extended sequence that end (width - 1) / 2 entries after position i;
// untouched for width < 3; the host admits width <= T only), threshold [c] = ((1 - weight) * lowest tenth).mean() + weight *
// highest tenth.mean() of prob, active = prob > threshold
__global__ __launch_bounds__(kThreads) void onset_threshold_kernel(OnsetDev m) {
    __shared__ int hist[kThreads], pick[2];
    __shared__ double red[kThreads];
    int *ired = hist;
    const int tid = threadIdx.x;
    const ClipRec C = m.clips[blockIdx.x];
    const int T = C.T, W = C.width, tenth = T / 10;
    const double *__restrict__ raw = m.raw + C.frame_off;
    double *prob = m.prob + C.frame_off;
    if (W < 3 || W > T) {
        for (int t = tid; t < T; t += kThreads) prob[t] = raw[t];
    } else {
        const double first = raw[0], last = raw[T - 1], box = 1.0 / (double)W;
        const int shift = 1 + (W - 1) / 2;
        for (int t = tid; t < T; t += kThreads) {
            double s = 0.0;
            for (int j = 0; j < W; ++j) {
                const int e = t + shift + j;            // index into lead [W] | raw [T] | trail [W - 1]
                double x;
                if (e < W) x = 2.0 * first - raw[W - 1 - e];
                else if (e < W + T) x = raw[e - W];
                else x = 2.0 * last - raw[T - 1 - (e - W - T)];
                s += x * box;
            }
            prob[t] = s;
        }
    }
    if (tenth < 1) {
        for (int t = tid; t < T; t += kThreads) m.active[C.frame_off + t] = 0;
        if (tid == 0) m.thr[blockIdx.x] = 0.0;
        return;
    }
    __syncthreads();                                    // prob is complete (written and read by this workgroup alone)
    const double v_lo = block_select(prob, T, tenth - 1, hist, pick, tid);
    const double v_hi = block_select(prob, T, T - tenth, hist, pick, tid);
    const double weight = C.weight, rest = 1.0 - weight;
    double s_lo = 0.0, s_hi = 0.0;
    int c_lo = 0, c_hi = 0;
    for (int t = tid; t < T; t += kThreads) {
        const double x = prob[t];
        if (x < v_lo) { s_lo += rest * x; ++c_lo; }
        if (x > v_hi) { s_hi += x; ++c_hi; }
    }
    s_lo = block_sum(s_lo, red, tid);
    s_hi = block_sum(s_hi, red, tid);
    c_lo = block_sum(c_lo, ired, tid);
    c_hi = block_sum(c_hi, ired, tid);
    const double low = s_lo + (double)(tenth - c_lo) * (rest * v_lo), high = s_hi + (double)(tenth - c_hi) * v_hi;
    const double thr = low / (double)tenth + weight * (high / (double)tenth);
    for (int t = tid; t < T; t += kThreads) m.active[C.frame_off + t] = prob[t] > thr;
    if (tid == 0) m.thr[blockIdx.x] = thr;
}

}  // namespace onset
}  // namespace paa
