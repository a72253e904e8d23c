// k-nearest-neighbour classification over many feature vectors: what audioTrainTest.Knn.classify (audioTrainTest.py:33-49)
// computes once per mid-term window (audioSegmentation.mid_term_file_classification, :586-591) or once per file
// (audioTrainTest.file_classification, :1091-1095) for the shipped knn_* models.  The reference takes the Euclidean distance
// to every training row (scipy cdist), argsorts it, counts the labels 0..n_classes-1 among the first `neighbors` rows and
// returns P[c] = count / neighbors and the first arg-max of P.
// Here the ranking is by squared distance in the difference form sum_d (t_d - x_d)^2 (no sqrt, no |x|^2 + |t|^2 - 2 x.t
// expansion, whose cancellation reorders close neighbours), ties broken by the training index: the order is ascending
// (d^2, index).  The reference's argsort leaves the order of equal distances undefined.
// One kernel per k (a template parameter, 1..kMaxK), on the lane split of kernels_kv.hpp with ONE query per group and the
// training rows as rows:
//  * per step of 8 rows each lane forms its partial squared distances to all 8, and a three-stage reduce-scatter (xor 4,
//    2, 1: 7 shuffles) leaves lane l with the full d^2 of row base + l;
//  * lane l keeps a sorted list of its K best (d^2, index) in registers for the rows = l mod 8; after warm-up a row costs
//    one compare against the list's last entry;
//  * at the end K rounds of a group arg-min merge the eight lists, the labels of the K neighbours are counted (lane l counts
//    classes l, l + 8, ...), P = count / K and the first maximum are written.
// NaN distances (a NaN query, i.e. a zero std) are never inserted: such a query gets P = 0, label 0 and no neighbours (-1).
#pragma once
#include "kernels_kv.hpp"
#include "model_launch.hpp"

namespace paa {
namespace knn {

using kv::kGroupLanes;
using kv::kMaxM;
using kv::kThreads;
using kv::kTile;
static_assert(kMaxDims <= kv::kMaxDims && kQueriesPerBlock * kGroupLanes == kThreads && kTile % kGroupLanes == 0,
              "one query per group; a tile is whole steps of 8 rows");
constexpr int kClassSlots = kMaxClasses / kGroupLanes;              // 8 classes per lane

// (d, i) before (e, j) in ascending (d^2, index) order; an index < 0 is an empty slot, after every real entry
__device__ __forceinline__ bool before(double d, int i, double e, int j) {
    if (j < 0) return i >= 0;
    if (i < 0) return false;
    return d < e || (d == e && i < j);
}

template <int K>
__global__ __launch_bounds__(kThreads) void knn_kernel(KnnDev m, const double *__restrict__ feats, long long ld, long long n_vec,
                                                       const double *__restrict__ mean, const double *__restrict__ scale,
                                                       int *__restrict__ label, double *__restrict__ proba,
                                                       int *__restrict__ neighbors) {
    extern __shared__ double tile[];                                // [kTile][pitch]
    const int tid = threadIdx.x, lane = tid % kGroupLanes, group = tid / kGroupLanes;
    const int M = (m.n_dims + kGroupLanes - 1) / kGroupLanes, pitch = M * kGroupLanes;
    const long long q = (long long)blockIdx.x * kQueriesPerBlock + group;
    const bool live = q < n_vec;
    double x[kMaxM];
#pragma unroll
    for (int i = 0; i < kMaxM; ++i) {
        const int d = lane + kGroupLanes * i;
        x[i] = (i < M && d < m.n_dims && live) ? (feats[(long long)d * ld + q] - mean[d]) / scale[d] : 0.0;
    }
    double dk[K];
    int ik[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { dk[j] = __builtin_inf(); ik[j] = -1; }

    for (int base = 0; base < m.n_train; base += kTile) {
        __syncthreads();
        kv::stage_rows(tile, m.train, base, m.n_train, m.n_dims, pitch, tid);
        __syncthreads();
        const int cnt = min(kTile, m.n_train - base);
        for (int r = 0; r < cnt; r += kGroupLanes) {
            const double *t = tile + r * pitch + lane;
            double p[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) p[j] = 0.0;
#pragma unroll
            for (int i = 0; i < kMaxM; ++i) {
                if (i < M) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const double df = t[j * pitch + kGroupLanes * i] - x[i];
                        p[j] = fma(df, df, p[j]);
                    }
                }
            }
            // reduce-scatter over the group: lane l ends with the sum over all 8 lanes of row r + l
            const bool b2 = lane & 4, b1 = lane & 2, b0 = lane & 1;
            double a[4], b[2];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double send = b2 ? p[j] : p[j + 4], keep = b2 ? p[j + 4] : p[j];
                a[j] = keep + __shfl_xor(send, 4, kGroupLanes);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const double send = b1 ? a[j] : a[j + 2], keep = b1 ? a[j + 2] : a[j];
                b[j] = keep + __shfl_xor(send, 2, kGroupLanes);
            }
            const double send = b0 ? b[0] : b[1], keep = b0 ? b[1] : b[0];
            const double d2 = keep + __shfl_xor(send, 1, kGroupLanes);
            const int row = base + r + lane;
            // this lane's rows arrive in ascending index order, so an equal d^2 never goes before a real entry; the
            // gate is false for NaN
            if (row < m.n_train && d2 <= dk[K - 1]) {
#pragma unroll
                for (int j = K - 1; j > 0; --j) {
                    if (d2 < dk[j - 1] || ik[j - 1] < 0) { dk[j] = dk[j - 1]; ik[j] = ik[j - 1]; }
                    else if (d2 < dk[j] || ik[j] < 0) { dk[j] = d2; ik[j] = row; }
                }
                if (d2 < dk[0] || ik[0] < 0) { dk[0] = d2; ik[0] = row; }
            }
        }
    }

    // merge the eight lists: K rounds of a group arg-min over the list heads; the winning lane pops its head
    int nb[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double wd = dk[0];
        int wi = ik[0];
#pragma unroll
        for (int o = 1; o < kGroupLanes; o <<= 1) {
            const double od = __shfl_xor(wd, o, kGroupLanes);
            const int oi = __shfl_xor(wi, o, kGroupLanes);
            if (before(od, oi, wd, wi)) { wd = od; wi = oi; }
        }
        nb[j] = wi;
        if (wi >= 0 && ik[0] == wi) {
#pragma unroll
            for (int s = 0; s + 1 < K; ++s) { dk[s] = dk[s + 1]; ik[s] = ik[s + 1]; }
            dk[K - 1] = __builtin_inf();
            ik[K - 1] = -1;
        }
    }
    // votes: lane l counts classes l + 8 s
    int votes[kClassSlots];
#pragma unroll
    for (int s = 0; s < kClassSlots; ++s) votes[s] = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int lab = nb[j] >= 0 ? m.labels[nb[j]] : -1;
#pragma unroll
        for (int s = 0; s < kClassSlots; ++s) votes[s] += lab == lane + kGroupLanes * s;
    }
    int key = -1;                                 // votes * 128 + (127 - class): the most votes, then the lowest class
#pragma unroll
    for (int s = 0; s < kClassSlots; ++s) {
        const int c = lane + kGroupLanes * s;
        if (c < m.n_classes) key = max(key, votes[s] * 128 + (127 - c));
    }
#pragma unroll
    for (int o = 1; o < kGroupLanes; o <<= 1) key = max(key, __shfl_xor(key, o, kGroupLanes));
    if (!live) return;
#pragma unroll
    for (int s = 0; s < kClassSlots; ++s) {
        const int c = lane + kGroupLanes * s;
        if (c < m.n_classes) proba[q * m.n_classes + c] = (double)votes[s] / (double)K;
    }
    if (lane == 0) label[q] = 127 - key % 128;
    if (neighbors) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j % kGroupLanes == lane) neighbors[q * K + j] = nb[j];
    }
}

// The sibling of kv::stage_rows for a job of a split sweep: tile [kTile][pitch] = the rows idx[base .. base + kTile - 1] of
// X [..][n_dims], each element standardised as (x - mean_d) / scale_d, zero beyond `end` and n_dims (the whole workgroup; the
// caller synchronises).  The division is IEEE: the tile holds exactly what StandardScaler.transform gives the reference.
__device__ __forceinline__ void stage_split_rows(double *tile, const double *X, const int *idx, int base, int end, int n_dims,
                                                 const double *mean, const double *scale, int pitch, int tid) {
    for (int i = tid; i < kTile * pitch; i += kThreads) {
        const int s = base + i / pitch;
        const int d = i % pitch;
#ifdef PAA_KNN_SPLIT_STAGE_MUL      // measurement only (scripts/bench_classify.py --train): what the division costs; answers differ in the last bit
        tile[i] = (s < end && d < n_dims) ? (X[(long long)idx[s] * n_dims + d] - mean[d]) * scale[d] : 0.0;
#else
        tile[i] = (s < end && d < n_dims) ? (X[(long long)idx[s] * n_dims + d] - mean[d]) / scale[d] : 0.0;
#endif
    }
}

// knn_kernel over the jobs of a split sweep (KnnSplitDev; audioTrainTest.evaluate_classifier :631-700 for "knn": per split a
// StandardScaler of the training rows, Knn.classify of every test row).  One workgroup serves 16 consecutive entries of ONE
// job's test list (m.blocks); what differs from knn_kernel:
//  * the query is row test_idx[..] of X and a training tile gathers rows train_idx[..] of X, both standardised on the load
//    path, element first: (x - mean_j) / scale_j, then the difference;
//  * the order is ascending (d^2, position in the job's train list) -- the reference's row index into X_train, not the
//    sample index; a lane's rows still arrive in ascending position, so the insertion rule is knn_kernel's;
//  * K is the launch's list length, >= every job's k: the merged list is a total order, so its first k_j entries are the job's
//    k_j nearest; they vote, P = votes / k_j, the label is the first maximum over the classes < n_classes_j, and a training
//    label >= n_classes_j counts for no class.
// P rows are max_classes wide (zeros at and beyond n_classes_j), neighbour rows K wide (-1 past k_j or the train list).
template <int K>
__global__ __launch_bounds__(kThreads) void knn_split_kernel(KnnSplitDev m, int *__restrict__ label, double *__restrict__ proba,
                                                             int *__restrict__ neighbors) {
    extern __shared__ double tile[];                                // [kTile][pitch]
    const int tid = threadIdx.x, lane = tid % kGroupLanes, group = tid / kGroupLanes;
    const int M = (m.n_dims + kGroupLanes - 1) / kGroupLanes, pitch = M * kGroupLanes;
    const SplitBlock blk = m.blocks[blockIdx.x];
    const long long t0 = m.train_off[blk.job], q0 = m.test_off[blk.job];
    const int n_train = (int)(m.train_off[blk.job + 1] - t0), n_test = (int)(m.test_off[blk.job + 1] - q0);
    const int kj = m.k[blk.job], n_classes = m.n_classes[blk.job];
    const double *__restrict__ mean = m.mean + (long long)blk.job * m.n_dims;
    const double *__restrict__ scale = m.scale + (long long)blk.job * m.n_dims;
    const int *__restrict__ train_idx = m.train_idx + t0;
    const int qi = blk.first + group;
    const bool live = qi < n_test;
    const long long q = q0 + qi;                                    // the query's place in the outputs
    const double *__restrict__ xrow = m.X + (long long)(live ? m.test_idx[q] : 0) * m.n_dims;
    double x[kMaxM];
#pragma unroll
    for (int i = 0; i < kMaxM; ++i) {
        const int d = lane + kGroupLanes * i;
        x[i] = (i < M && d < m.n_dims && live) ? (xrow[d] - mean[d]) / scale[d] : 0.0;
    }
    double dk[K];
    int ik[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { dk[j] = __builtin_inf(); ik[j] = -1; }

    for (int base = 0; base < n_train; base += kTile) {
        __syncthreads();
        stage_split_rows(tile, m.X, train_idx, base, n_train, m.n_dims, mean, scale, pitch, tid);
        __syncthreads();
        const int cnt = min(kTile, n_train - base);
        for (int r = 0; r < cnt; r += kGroupLanes) {
            const double *t = tile + r * pitch + lane;
            double p[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) p[j] = 0.0;
#pragma unroll
            for (int i = 0; i < kMaxM; ++i) {
                if (i < M) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const double df = t[j * pitch + kGroupLanes * i] - x[i];
                        p[j] = fma(df, df, p[j]);
                    }
                }
            }
            // reduce-scatter over the group: lane l ends with the sum over all 8 lanes of row r + l
            const bool b2 = lane & 4, b1 = lane & 2, b0 = lane & 1;
            double a[4], b[2];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double send = b2 ? p[j] : p[j + 4], keep = b2 ? p[j + 4] : p[j];
                a[j] = keep + __shfl_xor(send, 4, kGroupLanes);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const double send = b1 ? a[j] : a[j + 2], keep = b1 ? a[j + 2] : a[j];
                b[j] = keep + __shfl_xor(send, 2, kGroupLanes);
            }
            const double send = b0 ? b[0] : b[1], keep = b0 ? b[1] : b[0];
            const double d2 = keep + __shfl_xor(send, 1, kGroupLanes);
            const int row = base + r + lane;                        // position in the job's train list
            if (row < n_train && d2 <= dk[K - 1]) {
#pragma unroll
                for (int j = K - 1; j > 0; --j) {
                    if (d2 < dk[j - 1] || ik[j - 1] < 0) { dk[j] = dk[j - 1]; ik[j] = ik[j - 1]; }
                    else if (d2 < dk[j] || ik[j] < 0) { dk[j] = d2; ik[j] = row; }
                }
                if (d2 < dk[0] || ik[0] < 0) { dk[0] = d2; ik[0] = row; }
            }
        }
    }

    // merge the eight lists (as knn_kernel); only the first k_j entries vote
    int nb[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double wd = dk[0];
        int wi = ik[0];
#pragma unroll
        for (int o = 1; o < kGroupLanes; o <<= 1) {
            const double od = __shfl_xor(wd, o, kGroupLanes);
            const int oi = __shfl_xor(wi, o, kGroupLanes);
            if (before(od, oi, wd, wi)) { wd = od; wi = oi; }
        }
        nb[j] = j < kj ? wi : -1;
        if (wi >= 0 && ik[0] == wi) {
#pragma unroll
            for (int s = 0; s + 1 < K; ++s) { dk[s] = dk[s + 1]; ik[s] = ik[s + 1]; }
            dk[K - 1] = __builtin_inf();
            ik[K - 1] = -1;
        }
    }
    int votes[kClassSlots];
#pragma unroll
    for (int s = 0; s < kClassSlots; ++s) votes[s] = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int lab = nb[j] >= 0 ? m.labels[train_idx[nb[j]]] : -1;
#pragma unroll
        for (int s = 0; s < kClassSlots; ++s) votes[s] += lab == lane + kGroupLanes * s;
    }
    int key = -1;                                 // votes * 128 + (127 - class): the most votes, then the lowest class
#pragma unroll
    for (int s = 0; s < kClassSlots; ++s) {
        const int c = lane + kGroupLanes * s;
        if (c < n_classes) key = max(key, votes[s] * 128 + (127 - c));
    }
#pragma unroll
    for (int o = 1; o < kGroupLanes; o <<= 1) key = max(key, __shfl_xor(key, o, kGroupLanes));
    if (!live) return;
    if (proba) {
#pragma unroll
        for (int s = 0; s < kClassSlots; ++s) {
            const int c = lane + kGroupLanes * s;
            if (c < m.max_classes) proba[q * m.max_classes + c] = c < n_classes ? (double)votes[s] / (double)kj : 0.0;
        }
    }
    if (lane == 0) label[q] = 127 - key % 128;
    if (neighbors) {
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j % kGroupLanes == lane) neighbors[q * K + j] = nb[j];
    }
}

}  // namespace knn
}  // namespace paa
