"""Edges of the kNN kernel (pyaudioanalysis_amd/csrc/kernels_knn.hpp) against tests/knn_ref.py.  -m gpu.

Every case here is exact: training rows and queries are small integers fed with mean 0 and std 1, so every squared distance
is an exact integer in FP64 in whatever order the kernel's lanes add the squares, ascending (d^2, training index) is a total
order, and labels, P and the neighbour list must equal the restatement's with no vector set aside.  The cases sit on the
kernel's seams: n_train around the 8 lanes of a group and the 16-row LDS tile, k around 8 and at kMaxK, k > n_train
(missing neighbours are -1), n_dims around the 8-lane split and at kMaxDims, class counts around the 8 classes per lane
with classes that have no training row, n_vec around the 16 queries of a workgroup, a leading dimension above n_vec, and
queries whose distances are inf for all rows or for some.  That the cases really hold ties at the k-th place, between
the eight lists, between tiles and between classes is asserted on the CPU in tests/test_model_edges_ref_cpu.py."""
import numpy as np
import pytest

import knn_ref
from pyaudioanalysis_amd import _ffi, audioTrainTest

pytestmark = pytest.mark.gpu


def _predict(F, labels, k, X, ld=None, mean=None, std=None):
    """(labels, P, neighbours) of the rows of X through the host entry point, or the C ABI with ld > n_vec."""
    model = audioTrainTest.knn_model(audioTrainTest.Knn(F, labels, k))
    n_vec, n_dims = X.shape
    mean = np.zeros(n_dims) if mean is None else mean
    std = np.ones(n_dims) if std is None else std
    if ld is None:
        return model.predict(np.ascontiguousarray(X.T), mean, std, neighbors=True)
    M = np.full((n_dims, ld), 1e300)                              # the padding columns hold a value that would change d^2
    M[:, :n_vec] = X.T
    got = np.full(n_vec, -7, dtype=np.int32)
    P = np.full((n_vec, model.n_classes), -7.0)
    nb = np.full((n_vec, k), -7, dtype=np.int32)
    _ffi.check(_ffi.lib().paa_knn_predict_f64(model.handle, _ffi.as_f64p(M), n_dims, ld, n_vec, _ffi.as_f64p(mean),
                                              _ffi.as_f64p(std), got.ctypes.data_as(_ffi.c_i32p), _ffi.as_f64p(P),
                                              nb.ctypes.data_as(_ffi.c_i32p)))
    return got, P, nb


def _exact(F, labels, k, X, what, feats=None, **kw):
    """feats: what the kernel is fed where it is not X itself (X is then what the standardisation makes of it)."""
    got, P, nb = _predict(F, labels, k, X if feats is None else feats, **kw)
    want, wP, wnb = knn_ref.classify(F, labels, k, X)
    assert np.array_equal(nb, wnb), (what, "neighbours", np.flatnonzero((nb != wnb).any(axis=1))[:5])
    assert np.array_equal(P, wP), (what, "P")
    assert np.array_equal(got, want), (what, "labels")
    return got, P, nb


@pytest.mark.parametrize("n_train,k,n_dims,n_classes,n_vec", knn_ref.integer_grid())
def test_integer_grid_is_exact(gpu_lib, n_train, k, n_dims, n_classes, n_vec):
    F, labels, X = knn_ref.integer_case(n_train, n_dims, n_classes, n_vec, 1000 * n_train + k)
    got, P, nb = _exact(F, labels, k, X, (n_train, k, n_dims, n_classes, n_vec))
    assert P.shape == (n_vec, min(n_classes, n_train))
    assert np.all(nb[:, min(k, n_train):] == -1) and np.all(nb[:, :min(k, n_train)] >= 0)
    assert np.all(P[:, 1::2] == 0)                                # the odd classes have no training row
    # the same queries behind a leading dimension above n_vec
    _exact(F, labels, k, X, "ld", ld=n_vec + 5)


@pytest.mark.parametrize("n_dims", knn_ref.INT_DIMS)
@pytest.mark.parametrize("n_classes", knn_ref.INT_CLASSES)
def test_dims_and_classes(gpu_lib, n_dims, n_classes):
    """Every n_dims with every class count, on a model long enough (100 rows, 7 tiles) for all 64 classes; k = 9 > 8."""
    F, labels, X = knn_ref.integer_case(100, n_dims, n_classes, 17, 7 * n_dims + n_classes)
    got, P, nb = _exact(F, labels, 9, X, (n_dims, n_classes))
    assert P.shape == (17, n_classes)


@pytest.mark.parametrize("n_vec", knn_ref.INT_N_VEC)
@pytest.mark.parametrize("k", (1, 8, 32))
def test_tie_rich_case(gpu_lib, n_vec, k):
    """7 dims of -1..1 against 33 rows: a few distinct distances, so ties of all four kinds in nearly every query."""
    F, labels, X = knn_ref.integer_case(33, 7, 8, n_vec, 5)
    _exact(F, labels, k, X, (n_vec, k))
    _exact(F, labels, k, X, "ld", ld=n_vec + 48)


def test_duplicated_rows_and_queries_on_them(gpu_lib):
    """All 40 rows identical: every distance ties, the order is the index order alone; then two interleaved copies."""
    F = np.tile(np.array([[1.0, -1.0, 0.0]]), (40, 1))
    labels = (np.arange(40) % 3).astype(np.float64)
    X = np.array([[1.0, -1.0, 0.0], [0.0, 0.0, 0.0], [3.0, 3.0, 3.0]])
    for k in (1, 9, 32):
        got, P, nb = _exact(F, labels, k, X, k)
        assert np.array_equal(nb, np.tile(np.arange(k), (3, 1)))
    F[1::2] = [0.0, 0.0, 0.0]
    for k in (1, 9, 32):
        _exact(F, labels, k, X, k)


def test_vote_tie_goes_to_the_lowest_class(gpu_lib):
    """k = 4 over rows labelled 5, 5, 2, 2 nearest: classes 2 and 5 tie at two votes; also a three-way tie that includes
    class 0 and a tie among the last classes 62 and 63."""
    F = np.arange(200, dtype=np.float64)[:, None]
    labels = np.arange(200, dtype=np.float64) % 64
    labels[:4] = [5, 5, 2, 2]
    labels[10:16] = [63, 62, 63, 62, 9, 9]
    labels[30:36] = [7, 0, 3, 7, 3, 0]
    F[10:16] = 1000.0                                             # equal rows: the order among them is the index order
    F[30:36] = 2000.0
    assert np.unique(labels).shape[0] == 64
    X = np.array([[0.0], [1000.0], [2000.0]])
    got, P, nb = _exact(F, labels, 4, X[:2], "two-way")
    assert got.tolist() == [2, 62]
    got, P, nb = _exact(F, labels, 6, X[2:], "three-way")
    assert got.tolist() == [0] and P[0, [0, 3, 7]].tolist() == [2 / 6.0] * 3


def test_all_inf_query_takes_the_first_rows(gpu_lib):
    """x / 0 = +-inf in every dim: every squared distance is inf, the neighbours are rows 0..k-1 in index order."""
    F, labels, X = knn_ref.integer_case(33, 9, 8, 17, 11)
    feats = np.where(X == 0, 1.0, X)                              # no 0 / 0
    with np.errstate(divide="ignore"):
        Xinf = feats / np.zeros(9)
    assert np.isinf(Xinf).all()
    for k in (1, 8, 9, 32):
        got, P, nb = _exact(F, labels, k, Xinf, k, feats=feats, std=np.zeros(9))
        assert np.array_equal(nb, np.tile(np.arange(k), (17, 1)))
    # one dim alone at inf is enough
    std = np.ones(9)
    std[4] = 0.0
    with np.errstate(divide="ignore"):
        X1 = feats / std
    got, P, nb = _exact(F, labels, 9, X1, "one dim", feats=feats, std=std)
    assert np.array_equal(nb, np.tile(np.arange(9), (17, 1)))


def test_distances_that_overflow_for_some_rows(gpu_lib):
    F, labels, k, X = knn_ref.overflow_case()
    D = knn_ref.squared_distances(F, X)
    assert np.isinf(D).any(axis=1).all() and np.isfinite(D).any(axis=1).all()
    got, P, nb = _exact(F, labels, k, X, "overflow")
    for v in range(X.shape[0]):
        finite = int(np.isfinite(D[v]).sum())
        assert finite < k and np.isfinite(D[v, nb[v, :finite]]).all() and np.isinf(D[v, nb[v, finite:]]).all()
        assert np.all(np.diff(nb[v, finite:]) > 0)               # the inf rows follow in index order
