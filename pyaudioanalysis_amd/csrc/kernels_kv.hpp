// Kernel values of many feature vectors against the rows of a model: what svc_class_sums_kernel (kernels_svc.hpp),
// svr_bank_kernel (kernels_svr.hpp) and knn_kernel (kernels_knn.hpp) share.  Device code only.
// A group of kGroupLanes lanes owns W windows (feature vectors); lane l holds dims l, l + 8, l + 16, ... of each in
// registers, standardised on load and zero beyond n_dims (M = ceil(n_dims / 8) dims per lane, pitch = 8 M).  A workgroup
// stages tiles of kTile model rows (support vectors, training rows), zero-padded to `pitch` dims, in LDS: one read of a tile
// per workgroup.  Per row a lane forms its partial squared difference (RBF, kNN) or dot product (linear) over i < M -- the
// padding adds exact zeros -- and three xor shuffles give every lane of the group the full sum.  Every value is a
// fixed-order chain of fma's owned by one lane group: it depends neither on the window's place in the batch nor on n_vec.
// Here: the geometry, the group sum and the tile copy.  The standardise-on-load and the accumulation over a row stay written
// out in each kernel: as inline helpers shared by the three they compiled to the same instructions under another register
// allocation, and svc_class_sums_kernel ran 1.4 - 3.1 % slower, svr_bank_kernel 0.3 - 1.4 %, beyond
// the run-to-run spread (profiles/kv_refactor_ab.json); with the helpers below the three units' machine code is unchanged.
#pragma once
#include <hip/hip_runtime.h>

namespace paa {
namespace kv {

constexpr int kGroupLanes = 8;
constexpr int kThreads = 128;                                         // 16 groups
constexpr int kTile = 16;                                             // model rows per LDS tile
constexpr int kMaxDims = 256;
constexpr int kMaxM = kMaxDims / kGroupLanes;                         // 32 dims per lane

__device__ __forceinline__ double group_sum(double v) {
    v += __shfl_xor(v, 1, kGroupLanes);
    v += __shfl_xor(v, 2, kGroupLanes);
    v += __shfl_xor(v, 4, kGroupLanes);
    return v;
}

// tile [kTile][pitch] = rows base .. base + kTile - 1 of rows [end][n_dims], zero beyond `end` and n_dims (the whole
// workgroup; the caller synchronises).  I: the caller's row index type.  n_dims comes by reference: by value the copy is
// simplified on its own before it is inlined, and svr_bank_kernel's machine code moves (same work, other registers)
template <typename I>
__device__ __forceinline__ void stage_rows(double *tile, const double *rows, I base, I end, const int &n_dims, int pitch, int tid) {
    for (int i = tid; i < kTile * pitch; i += kThreads) {
        const I s = base + i / pitch;
        const int d = i % pitch;
        tile[i] = (s < end && d < n_dims) ? rows[(long long)s * n_dims + d] : 0.0;
    }
}

}  // namespace kv
}  // namespace paa
