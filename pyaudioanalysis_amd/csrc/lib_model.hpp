// What the model families (lib_svc / knn / forest / hmm / diar.hpp) share on the host: the 256-byte rounding of every
// sub-buffer, the feature-matrix argument test, the device block of a model handle, the staging of a host-buffer call
// through a lane, and the launch-failure return.  No device code.
#pragma once

static inline size_t up256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// `what launch failed: <HIP error>` when a launch:: entry point reports a failure
#define LAUNCH_TRY(what, call)                                                                                   \
    do {                                                                                                         \
        if (call) return fail(PAA_ERR_HIP, what " launch failed: %s", hipGetErrorString(hipGetLastError()));     \
    } while (0)

// A feature matrix [n_dims][ld] with n_vec columns in use: model_check<Handle> against the n_dims of the model behind the
// handle (PaaSvc, PaaSvr, PaaKnn, PaaForest, PaaHmm), or check_matrix for an entry point without a model; max_vec: the
// family's grid limit (0: none).  Runs before ensure_init(): an argument error is reported on a host without a device too.
static int check_matrix(int64_t ld, int64_t n_vec, int64_t max_vec) {
    if (n_vec < 1 || ld < n_vec) return fail(PAA_ERR_ARG, "bad feature matrix: %lld vectors, ld %lld", (long long)n_vec, (long long)ld);
    if (max_vec && n_vec > max_vec) return fail(PAA_ERR_ARG, "too many vectors");
    return PAA_OK;
}
template <typename Handle>
static int model_check(const void *handle, int n_dims, int64_t ld, int64_t n_vec, int64_t max_vec) {
    if (!handle) return fail(PAA_ERR_ARG, "null handle");
    const int model_dims = ((const Handle *)handle)->dev.n_dims;
    if (n_dims != model_dims) return fail(PAA_ERR_ARG, "feature vectors have %d dims, the model %d", n_dims, model_dims);
    return check_matrix(ld, n_vec, max_vec);
}

// The one device allocation behind a model handle: freed with the handle, also when its creation fails half way.
struct DevBlock {
    void *p = nullptr;
    DevBlock() = default;
    DevBlock(const DevBlock &) = delete;
    DevBlock &operator=(const DevBlock &) = delete;
    ~DevBlock() { if (p) (void)hipFree(p); }
};
struct BlockPart {
    const void *src;        // host array
    size_t bytes, align;
    void *dev;              // out: its place in the block
};
// allocates b for the parts in order, each at its alignment, and uploads them (a part without a source is room only); `what`
// names the model in the error message
static int block_upload(DevBlock &b, BlockPart *parts, int n, const char *what) {
    size_t total = 0;
    for (int i = 0; i < n; ++i) total = (total + parts[i].align - 1) / parts[i].align * parts[i].align + parts[i].bytes;
    HIP_TRY(hipMalloc(&b.p, total));
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        at = (at + parts[i].align - 1) / parts[i].align * parts[i].align;
        parts[i].dev = (char *)b.p + at;
        if (parts[i].src && hipMemcpy(parts[i].dev, parts[i].src, parts[i].bytes, hipMemcpyHostToDevice) != hipSuccess)
            return fail(PAA_ERR_HIP, "uploading %s failed", what);
        at += parts[i].bytes;
    }
    return PAA_OK;
}
// paa_*_destroy: frees the block (and `also`, the HMM's work buffer) and deletes the handle; the first hipFree error is reported
template <typename Handle>
static int model_destroy(Handle *h, void *also = nullptr) {
    if (!h) return PAA_OK;
    hipError_t e = h->block.p ? hipFree(h->block.p) : hipSuccess;
    h->block.p = nullptr;
    if (also) {
        const hipError_t e2 = hipFree(also);
        if (e == hipSuccess) e = e2;
    }
    delete h;
    return e == hipSuccess ? PAA_OK : fail(PAA_ERR_HIP, "hipFree: %s", hipGetErrorString(e));
}

// One host-buffer call in a lane: stage() reserves the lane's scratch (in: feats | mean | std, mean / std optional; mid:
// the family's work space; out: every output but the last padded to 256 B), issues the host-to-device copies and fills the
// device pointers; after the launches finish() issues the device-to-host copies and synchronises.  An output with a null
// host pointer is not wanted: its device pointer is null and nothing is copied back.
struct HostOut {
    void *host;
    size_t bytes;
};
constexpr int kMaxStagedOuts = 3;
struct Staged {
    LaneGuard lane;       // own stream + scratch for this call (see Lane)
    double *feats = nullptr, *mean = nullptr, *std = nullptr;
    void *mid = nullptr;
    void *out[kMaxStagedOuts] = {nullptr, nullptr, nullptr};
    HostOut outs[kMaxStagedOuts] = {};
    int n_out = 0;
};
static int stage(Staged &s, const double *feats, int n_dims, int64_t ld, const double *mean, const double *std, size_t mid_bytes,
                 std::initializer_list<HostOut> outs) {
    const size_t fb = (size_t)n_dims * ld * 8, sb = (size_t)n_dims * 8;
    size_t off[kMaxStagedOuts], out_bytes = 0;
    for (const HostOut &o : outs) {
        off[s.n_out] = up256(out_bytes);
        out_bytes = off[s.n_out] + (o.host ? o.bytes : 0);
        s.outs[s.n_out++] = o;
    }
    Lane &l = *s.lane.l;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        int rc;
        if ((rc = scratch_reserve(l.in, fb + (mean ? 2 * sb : 0)))) return rc;
        if ((rc = scratch_reserve(l.mid, mid_bytes))) return rc;
        if ((rc = scratch_reserve(l.out, out_bytes))) return rc;
    }
    s.feats = (double *)l.in.p;
    s.mid = l.mid.p;
    for (int i = 0; i < s.n_out; ++i) s.out[i] = s.outs[i].host ? (char *)l.out.p + off[i] : nullptr;
    HIP_TRY(hipMemcpyAsync(s.feats, feats, fb, hipMemcpyHostToDevice, cs()));
    if (mean) {
        s.mean = s.feats + (size_t)n_dims * ld;
        s.std = s.mean + n_dims;
        HIP_TRY(hipMemcpyAsync(s.mean, mean, sb, hipMemcpyHostToDevice, cs()));
        HIP_TRY(hipMemcpyAsync(s.std, std, sb, hipMemcpyHostToDevice, cs()));
    }
    return PAA_OK;
}
static int finish(Staged &s) {
    for (int i = 0; i < s.n_out; ++i)
        if (s.out[i]) HIP_TRY(hipMemcpyAsync(s.outs[i].host, s.out[i], s.outs[i].bytes, hipMemcpyDeviceToHost, cs()));
    HIP_TRY(hipStreamSynchronize(cs()));
    return PAA_OK;
}
