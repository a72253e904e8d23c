"""Edges of the diarization kernels (pyaudioanalysis_amd/csrc/kernels_diar.hpp) against tests/diar_ref.py.  -m gpu.

pair_kernel: N on and around its 128-window tiles with D on and around its 8-dim panels, eight k in one launch over
hand-made labels that hold an empty cluster, a one-window cluster and a cluster wholly inside one tile, against
np.longdouble.  dimdist_kernel: D around its 16-row tiles over labelled subsets that are empty or hold one window.
standardize_kernel: nearly constant rows and rows under a large offset, the constant-feature decision where the CPU suite
has shown its margin.  k-means: designed inputs of small dyadic numbers on which every distance, sum and centre is exact
(diar_ref.equidistant_case, two_empty_case; exactness is asserted on the CPU in tests/test_model_edges_ref_cpu.py), so the
lowest-index rule of assign_kernel on equidistant centres and of finish_kernel on equally far windows shows in labels and
centres that are compared bit for bit.  Needs neither SciPy nor scikit-learn."""
import numpy as np
import pytest

import diar_ref
from pyaudioanalysis_amd import _ffi
from pyaudioanalysis_amd import audioSegmentation as aS

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
DIST_FLOOR = 1e-6
# Conditioning (the similarity suite's recipe): where the quantity is tiny against the data it is made from -- the variance
# under a large offset, the pair sum of near-duplicates -- the kernel may be K_COND x as far (relatively) from the longdouble
# reference as the FP64 restatement is, plus a floor of a few ulp.  K_COND is the smallest power of two that is at least
# twice the largest kernel / restatement ratio recorded in profiles/r08_model_edge_errors.json.
K_COND = 2
COND_FLOOR = 8 * 2.220446049250313e-16


def _rel(got, ref):
    """Largest elementwise error relative to max(|ref|, 1); the NaN patterns must agree."""
    r64 = np.asarray(ref, dtype=np.float64)
    assert got.shape == r64.shape and np.array_equal(np.isnan(got), np.isnan(r64)), (got.shape, r64.shape)
    ok = ~np.isnan(r64)
    if not ok.any():
        return 0.0
    e = np.abs(got[ok] - np.asarray(ref)[ok]) / np.maximum(np.abs(np.asarray(ref)[ok]), 1.0)
    return float(np.max(e))


def _pure_rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def device_pair_sums(X, labels, ks):
    """paa_diar_dev_pair_sums_f64 on X [D][N] and labels [nk][N]."""
    lib = _ffi.lib()
    d_x, d_l = _ffi.DeviceBuffer.from_host(X), _ffi.DeviceBuffer.from_host(np.ascontiguousarray(labels, dtype=np.int32))
    ks_arr = np.array(ks, dtype=np.int32)
    out = np.empty((len(ks), 32, 32))
    try:
        _ffi.check(lib.paa_diar_dev_pair_sums_f64(d_x.ptr, X.shape[0], X.shape[1], X.shape[1], d_l.ptr,
                                                  ks_arr.ctypes.data_as(_ffi.c_i32p), len(ks), _ffi.as_f64p(out)))
    finally:
        d_x.free()
        d_l.free()
    return [out[i, :k, :k] for i, k in enumerate(ks)]


def device_kmeans(X, ks, inits, max_iter=300, tol=1e-4):
    """paa_diar_dev_kmeans_f64 on X [D][N]: per k (labels, centres, n_iter, inertia)."""
    lib = _ffi.lib()
    D, n = X.shape
    centers = np.zeros((len(ks), 32, D))
    for i, k in enumerate(ks):
        centers[i, :k] = inits[i]
    ks_arr = np.array(ks, dtype=np.int32)
    n_iter, inertia = np.zeros(len(ks), dtype=np.int32), np.empty(len(ks))
    d_x, d_l = _ffi.DeviceBuffer.from_host(np.ascontiguousarray(X)), _ffi.DeviceBuffer(len(ks) * n * 4)
    try:
        _ffi.check(lib.paa_diar_dev_kmeans_f64(d_x.ptr, D, n, n, ks_arr.ctypes.data_as(_ffi.c_i32p), len(ks), _ffi.as_f64p(centers),
                                               tol * float(np.mean(np.var(X, axis=1))), max_iter, d_l.ptr,
                                               n_iter.ctypes.data_as(_ffi.c_i32p), _ffi.as_f64p(inertia)))
        labels = d_l.to_host(np.int32, len(ks) * n).reshape(len(ks), n)
    finally:
        d_x.free()
        d_l.free()
    return [(labels[i].astype(np.int64), centers[i, :k].copy(), int(n_iter[i]), float(inertia[i])) for i, k in enumerate(ks)]


def device_dim_distances(Z, labels, ks):
    """paa_diar_dev_dim_distances_f64 on Z [D][N] over the label subsets: (colsum [nk][kmax][D], pmean [nk][kmax])."""
    lib = _ffi.lib()
    D, n = Z.shape
    kmax = max(ks)
    d_z, d_l = _ffi.DeviceBuffer.from_host(Z), _ffi.DeviceBuffer.from_host(np.ascontiguousarray(labels, dtype=np.int32))
    ks_arr = np.array(ks, dtype=np.int32)
    cols, pmean = np.full((len(ks), kmax, D), -7.0), np.full((len(ks), kmax), -7.0)
    try:
        _ffi.check(lib.paa_diar_dev_dim_distances_f64(d_z.ptr, D, n, n, d_l.ptr, ks_arr.ctypes.data_as(_ffi.c_i32p), len(ks),
                                                      _ffi.as_f64p(cols), _ffi.as_f64p(pmean)))
    finally:
        d_z.free()
        d_l.free()
    return cols, pmean


def device_standardize(X):
    lib = _ffi.lib()
    D, n = X.shape
    d_m, d_z = _ffi.DeviceBuffer.from_host(X), _ffi.DeviceBuffer(D * n * 8)
    stats = np.empty((3, D))
    try:
        _ffi.check(lib.paa_diar_dev_standardize_f64(d_m.ptr, D, n, n, d_z.ptr, _ffi.as_f64p(stats)))
        Z = d_z.to_host(np.float64, D * n).reshape(D, n)
    finally:
        d_m.free()
        d_z.free()
    return stats, Z


@pytest.mark.parametrize("D", [1, 7, 8, 9, 15, 16, 17, 33])
@pytest.mark.parametrize("n", [127, 128, 129, 255, 256, 257])
def test_pair_sums_on_tile_edges_eight_k_at_once(gpu_lib, n, D):
    rng = np.random.default_rng(1000 * n + D)
    X = np.ascontiguousarray(rng.standard_normal((D, n)) * 1.5)
    ks = list(diar_ref.PAIR_KS)
    labels = diar_ref.hand_labels(n, ks)
    S = device_pair_sums(X, labels, ks)
    worst = 0.0
    for i, k in enumerate(ks):
        want = diar_ref.pair_sums_p(X.T, labels[i], k)
        worst = max(worst, _rel(S[i], want))
        if k > 2:
            assert np.all(S[i][k - 1] == 0) and np.all(S[i][:, k - 1] == 0)      # the empty cluster
        assert S[i][1, 1] == 0.0                                              # the one-window cluster
        assert np.array_equal(S[i], S[i].T) or _rel(S[i], S[i].T) <= TIGHT
    print("pair sums n %d D %d: worst err %.3g" % (n, D, worst))
    assert worst <= TIGHT
    # one k alone gives the same bits as that k among eight
    alone = device_pair_sums(X, labels[5:6], ks[5:6])[0]
    assert alone.tobytes() == S[5].tobytes()


def test_pair_sums_of_near_duplicates(gpu_lib):
    """A cluster of windows 1e-9 apart among ordinary ones: its own pair sum is of the order of 1e-6, which the gate relative
    to max(|ref|, 1) cannot see; the FP64 restatement's own relative error is the yardstick."""
    X, labels = diar_ref.near_duplicate_case()
    S = device_pair_sums(X, labels[None, :], [3])[0]
    ld = diar_ref.pair_sums_p(X.T, labels, 3)
    f64 = diar_ref.pair_sums_p(X.T, labels, 3, np.float64)
    assert _rel(S, ld) <= TIGHT
    err_k, err_r = _pure_rel(S[2, 2], ld[2, 2]), _pure_rel(f64[2, 2], ld[2, 2])
    print("near-duplicate pair sum %.3g: kernel rel err %.3g, FP64 restatement %.3g, ratio %.3g"
          % (S[2, 2], err_k, err_r, err_k / max(err_r, 1e-300)))
    assert err_k <= K_COND * err_r + COND_FLOOR, (err_k, err_r)


@pytest.mark.parametrize("D", [1, 7, 8, 9, 15, 16, 17, 33])
def test_dimension_distances_over_small_and_empty_subsets(gpu_lib, D):
    n = 70
    rng = np.random.default_rng(D)
    Z = np.ascontiguousarray(rng.standard_normal((D, n)))
    labels = np.zeros((2, n), dtype=np.int32)
    labels[0, 40] = 1                       # k = 3: cluster 1 one window, cluster 2 empty
    labels[1] = np.arange(n) % 4            # k = 5: four even clusters, cluster 4 empty
    labels[1, 64:] = 3                      # ... the windows past the 64-window staging step all in one cluster
    ks = [3, 5]
    cols, pmean = device_dim_distances(Z, labels, ks)
    for i, k in enumerate(ks):
        for c in range(k):
            wcol, wmean = diar_ref.dim_distances_p(Z.T, labels[i] == c)
            assert _rel(cols[i, c], wcol) <= TIGHT, (D, k, c)
            assert _rel(pmean[i, c:c + 1], np.array([wmean])) <= TIGHT, (D, k, c, pmean[i, c], wmean)
        assert np.all(cols[i, k - 1] == 0)
    assert _rel(cols[0, 1], np.abs(Z[:, 40][:, None] - Z[:, 40][None, :]).sum(axis=0)) <= TIGHT


def test_scaler_on_nearly_constant_and_offset_rows(gpu_lib):
    worst = 0.0
    for n in (255, 256, 257, 300):
        X, constant = diar_ref.scaler_rows(n)
        stats, Z = device_standardize(X)
        mean, var, scale, c_ld, bound = diar_ref.standardize_p(X)
        assert np.array_equal(c_ld, constant)
        assert np.array_equal(stats[2] == 1.0, constant), (n, stats[2])       # the decision; margins shown on the CPU
        assert np.all(Z[constant] == (X[constant] - stats[0][constant][:, None]))
        assert _rel(stats[0], mean) <= TIGHT and _rel(stats[1], var) <= TIGHT and _rel(stats[2], scale) <= TIGHT
        m64, v64, s64, _, _ = diar_ref.standardize_p(X, np.float64)
        live = ~constant
        for name, got, ref64, ref in (("var", stats[1], v64, var), ("scale", stats[2], s64, scale)):
            err_k, err_r = _pure_rel(got[live], ref[live]), _pure_rel(ref64[live], ref[live])
            worst = max(worst, err_k / max(err_r, 1e-300))
            print("scaler n %d %s: kernel rel err %.3g, FP64 restatement %.3g" % (n, name, err_k, err_r))
            assert err_k <= K_COND * err_r + COND_FLOOR, (n, name, err_k, err_r)
        zref = ((np.asarray(X, dtype=np.longdouble) - mean[:, None]) / scale[:, None])
        assert _rel(Z[:1], zref[:1]) <= TIGHT
        # under an offset of 1e8 the FP64 mean is 1e-8 off, more than TIGHT x scale: Z of those rows cannot be held against
        # longdouble.  It is the two rounded operations (x - mean) / scale on the mean and scale the kernel reports: bit for bit
        assert Z.tobytes() == ((X - stats[0][:, None]) / stats[2][:, None]).tobytes(), n
    print("scaler: worst ratio %.3g" % worst)


@pytest.mark.parametrize("lead", [0, 1, 6])
def test_equidistant_centres_go_to_the_lowest_index(gpu_lib, lead):
    Z, init = diar_ref.equidistant_case(lead)
    k = init.shape[0]
    ref = diar_ref.kmeans(Z, k, init)
    labels, centers, n_iter, inertia = device_kmeans(np.ascontiguousarray(Z.T), [k], [init])[0]
    tied = (Z[:, 1] == 4.0)
    assert tied.sum() == 64 and np.all(labels[tied] == lead)
    assert np.array_equal(labels, ref["labels"]) and n_iter == ref["n_iter"] == 2
    assert centers.tobytes() == ref["centers"].tobytes() and inertia == ref["inertia"] == 960.0


def test_equidistant_centres_in_a_sweep_of_eight(gpu_lib):
    """Eight runs in one launch (the runs that are done drop out of later iterations): the six leading centres rotated, the
    tied pair at indices 6 and 7 throughout; then cut to k = 8 .. 2 by dropping leading centres with their windows."""
    Z, init = diar_ref.equidistant_case(6)
    inits = [np.vstack([np.roll(init[:6], i, axis=0), init[6:]]) for i in range(8)]
    got = device_kmeans(np.ascontiguousarray(Z.T), [8] * 8, inits)
    for (labels, centers, n_iter, inertia), ini in zip(got, inits):
        ref = diar_ref.kmeans(Z, 8, ini)
        assert np.array_equal(labels, ref["labels"]) and n_iter == ref["n_iter"] == 2
        assert np.all(labels[Z[:, 1] == 4.0] == 6)
        assert centers.tobytes() == ref["centers"].tobytes() and inertia == ref["inertia"]


def test_two_empty_clusters_take_the_farthest_windows_lowest_index_first(gpu_lib):
    Z, init = diar_ref.two_empty_case()
    ref = diar_ref.kmeans(Z, 4, init, max_iter=1)
    labels, centers, n_iter, inertia = device_kmeans(np.ascontiguousarray(Z.T), [4], [init], max_iter=1)[0]
    assert n_iter == 1
    assert centers[2].tolist() == list(diar_ref.FAR_TIES[5]) and centers[3].tolist() == list(diar_ref.FAR_TIES[6])
    assert centers.tobytes() == ref["centers"].tobytes()
    assert np.array_equal(labels, ref["labels"]) and labels[[5, 6, 133, 262]].tolist() == [2, 3, 0, 2]
    assert inertia == ref["inertia"]
    # run on to convergence: the restatement's labels and iteration count (every later decision clears the floor or is an
    # exact tie between the coincident windows)
    full = diar_ref.kmeans(Z, 4, init)
    labels, centers, n_iter, inertia = device_kmeans(np.ascontiguousarray(Z.T), [4], [init])[0]
    assert np.array_equal(labels, full["labels"]) and n_iter == full["n_iter"]
    assert _rel(centers, full["centers"]) <= TIGHT and _rel(np.array([inertia]), np.array([full["inertia"]])) <= TIGHT


def test_stage_dictionary_against_longdouble(gpu_lib):
    """diarize_clusters_device on N = 257, D = 17: scaler statistics, dimension-distance sums, the kept dimensions (margin
    asserted on the CPU), and centres and inertia of the sweep's k against the longdouble Lloyd from the same centres."""
    X, inits = diar_ref.stage_case()
    d_m = _ffi.DeviceBuffer.from_host(X)
    try:
        det, d_z = aS.diarize_clusters_device(d_m, X.shape[0], X.shape[1], 3, init_centers={3: inits})
        Z = d_z.to_host(np.float64, X.size).reshape(X.shape)
        d_z.free()
    finally:
        d_m.free()
    mean, var, scale, _, _ = diar_ref.standardize_p(X)
    assert _rel(det["mean"], mean) <= TIGHT and _rel(det["var"], var) <= TIGHT and _rel(det["scale"], scale) <= TIGHT
    Zld = (np.asarray(X, dtype=np.longdouble) - mean[:, None]) / scale[:, None]
    assert _rel(Z, Zld) <= TIGHT
    colsum, _ = diar_ref.dim_distances_p(Zld.T)
    assert _rel(det["dim_colsum"], colsum) <= TIGHT
    kept = np.nonzero(colsum < 1.1 * colsum.mean())[0]
    assert np.array_equal(det["kept_dims"], kept)
    ref = diar_ref.kmeans(Zld.T[:, kept], 3, inits, dtype=np.longdouble)
    assert ref["margin"] >= DIST_FLOOR
    assert np.array_equal(det["labels"][3], ref["labels"]) and det["n_iter"][3] == ref["n_iter"]
    assert _rel(det["centers"][3], ref["centers"]) <= TIGHT
    assert _rel(np.array([det["inertia"][3]]), np.array([ref["inertia"]])) <= TIGHT
    assert _rel(det["pair_sums"][3], diar_ref.pair_sums_p(Zld.T[:, kept], ref["labels"], 3)) <= TIGHT
