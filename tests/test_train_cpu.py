"""CPU-side checks of classifier tuning and training (audioTrainTest.evaluate_classifier / extract_features_and_train, the kNN
split sweep of kernels_knn.hpp): the NumPy restatement (tests/train_ref.py) against the train_* goldens of the unmodified
reference (scripts/make_train_golden.py), the facts about scikit-learn's splits the product relies on, the argument errors of
paa_knn_splits_f64 (reported before any device work) and the error returns of the Python entry points.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import knn_ref
import train_ref
from pyaudioanalysis_amd import _ffi, audioTrainTest

KNN_RUNS = [("train_knn_three", r) for r in ("r0_", "r1_")] + [("train_knn_rare", r) for r in ("r0_", "r1_", "r2_", "r3_")]
SKLEARN_RUNS = ["r%d_" % i for i in range(5)]


def _names(g):
    return [str(s) for s in g["class_names"]]


def _same(g, r, ret, cms, preds, text):
    assert ret == g[r + "ret"]
    assert np.array_equal(cms, g[r + "cms"])
    assert np.array_equal(np.concatenate(preds), g[r + "pred"])
    assert text == str(g[r + "text"])


def test_goldens_hold_what_the_checks_need():
    three, rare = train_ref.load_golden("train_knn_three"), train_ref.load_golden("train_knn_rare")
    assert tuple(three["class_sizes"]) == train_ref.THREE_SIZES and three["features"].shape == (135, train_ref.THREE_DIMS)
    assert tuple(rare["class_sizes"]) == train_ref.RARE_SIZES and rare["features"].shape == (47, train_ref.RARE_DIMS)
    assert three["params"].tolist() == train_ref.KNN_PARAMS and rare["params"].tolist() == [1, 3, 5]
    assert [(int(three[r + "mode"]), int(three[r + "n_exp"])) for r in train_ref.golden_runs(three)] == [(0, 4), (1, 4)]
    assert [(int(rare[r + "has_ids"]), int(rare[r + "mode"]), int(rare[r + "n_exp"])) for r in train_ref.golden_runs(rare)] == \
        [(0, 0, 6), (0, 1, 6), (1, 0, 6), (1, 1, 6)]
    # the seeded generators are the goldens' data
    assert np.array_equal(np.vstack(train_ref.three_class_features()), three["features"])
    assert np.array_equal(np.vstack(train_ref.rare_class_features()), rare["features"])
    # the rare case drives the missing-class repair: some split's test rows and predictions lack a class
    y = train_ref.features_to_matrix(train_ref.golden_features(rare))[1]
    lacking = 0
    for r in train_ref.golden_runs(rare):
        off = rare[r + "test_off"]
        for s, (tr, te, _, _) in enumerate(train_ref.run_splits(rare, r)):
            lacking += len(set(y[te].tolist()) | set(rare[r + "pred"][off[s]:off[s + 1]].tolist())) < 4
            assert np.unique(y[tr]).shape[0] <= 4
    assert lacking > 0
    sk = train_ref.load_golden("train_sklearn_small")
    assert [str(sk[r + "kind_name"]) for r in train_ref.golden_runs(sk)] == ["svm", "svm_rbf", "randomforest", "extratrees", "gradientboosting"]
    d = train_ref.load_golden("train_dir_small")
    assert d["saved_features"].shape[1] == 136 and d["saved_labels"].shape[0] == d["saved_features"].shape[0]


@pytest.mark.parametrize("name,r", KNN_RUNS)
def test_restatement_equals_the_reference_knn(name, r):
    g = train_ref.load_golden(name)
    n_exp = int(g[r + "n_exp"])
    out = train_ref.evaluate(train_ref.golden_features(g), _names(g), g["params"], int(g[r + "mode"]), n_exp,
                             train_ref.listed_split_source(train_ref.run_splits(g, r), n_exp), train_ref.knn_fit, train_ref.knn_classify)
    _same(g, r, *out)


@pytest.mark.parametrize("r", SKLEARN_RUNS)
def test_restatement_equals_the_reference_sklearn_types(r):
    sklearn = pytest.importorskip("sklearn")
    g = train_ref.load_golden("train_sklearn_small")
    if sklearn.__version__ != str(g["sklearn_version"]):
        pytest.skip("golden fitted by scikit-learn %s, installed %s: the fits need not agree" % (g["sklearn_version"], sklearn.__version__))
    feats = train_ref.golden_features(g)
    kind = str(g[r + "kind_name"])
    np.random.seed(int(g[r + "seed"]))
    out = train_ref.evaluate(feats, _names(g), g[r + "params"], int(g[r + "mode"]), int(g[r + "n_exp"]),
                             train_ref.random_split_source(sum(len(f) for f in feats), float(g[r + "train_percentage"])),
                             train_ref.sklearn_fit(kind), train_ref.sklearn_classify)
    _same(g, r, *out)
    assert np.array_equal(np.random.get_state()[1], g[r + "rng_after"]) and np.random.get_state()[2] == int(g[r + "rng_pos_after"])


@pytest.mark.parametrize("name", ["train_knn_three", "train_knn_rare"])
def test_no_knn_golden_query_is_ambiguous(name):
    """A condition of the exact comparisons with the reference: no test vector of any job has rows tied at its k-th
    distance with different labels on both sides (knn_ref.ambiguous).  ZERO may be set aside."""
    g = train_ref.load_golden(name)
    X, y = train_ref.features_to_matrix(train_ref.golden_features(g))
    total = 0
    for r in train_ref.golden_runs(g):
        for tr, te, mean, scale, k in train_ref.run_jobs(g, r):
            assert not knn_ref.ambiguous_vectors((X[tr] - mean) / scale, y[tr], k, (X[te] - mean) / scale).any()
            total += len(te)
    assert total >= 448


def test_index_split_equals_array_split():
    """train_test_split over np.arange(n) consumes NumPy's global state as the split of (X, y) does and gives its rows."""
    pytest.importorskip("sklearn")
    from sklearn.model_selection import train_test_split
    X, y = train_ref.features_to_matrix(train_ref.three_class_features())
    for seed, pct in ((1, 0.9), (2, 0.8), (3, 0.5)):
        np.random.seed(seed)
        X_train, X_test, y_train, y_test = train_test_split(X, y, test_size=1 - pct)
        after = np.random.get_state()
        np.random.seed(seed)
        tr, te = audioTrainTest._draw_split(X.shape[0], pct)
        again = np.random.get_state()
        assert np.array_equal(X[tr], X_train) and np.array_equal(X[te], X_test)
        assert np.array_equal(y[tr], y_train) and np.array_equal(y[te], y_test)
        assert np.array_equal(after[1], again[1]) and after[2] == again[2]


@pytest.mark.parametrize("name,r", KNN_RUNS)
def test_knn_splits_drawn_up_front_are_the_references(name, r):
    """All splits of a kNN sweep drawn before anything else (parameter-major; with ids the shared GroupShuffleSplit lists
    once): the reference's index lists and scalers, and the global state ends where the reference leaves it."""
    pytest.importorskip("sklearn")
    from sklearn.model_selection import GroupShuffleSplit
    from sklearn.preprocessing import StandardScaler
    g = train_ref.load_golden(name)
    X, y = train_ref.features_to_matrix(train_ref.golden_features(g))
    n_exp, n_params, ids = int(g[r + "n_exp"]), len(g["params"]), train_ref.run_ids(g, r)
    np.random.seed(int(g[r + "seed"]))
    if ids:
        shared = list(GroupShuffleSplit(n_splits=n_exp, train_size=.8).split(X, y, ids))
        drawn = [shared[e] for _ in range(n_params) for e in range(n_exp)]
    else:
        drawn = [audioTrainTest._draw_split(X.shape[0], float(g[r + "train_percentage"])) for _ in range(n_params * n_exp)]
    assert np.array_equal(np.random.get_state()[1], g[r + "rng_after"]) and np.random.get_state()[2] == int(g[r + "rng_pos_after"])
    for (tr, te), (gtr, gte, mean, scale) in zip(drawn, train_ref.run_splits(g, r)):
        assert np.array_equal(tr, gtr) and np.array_equal(te, gte)
        sc = StandardScaler().fit(X[tr])
        assert np.array_equal(sc.mean_, mean) and np.array_equal(sc.scale_, scale)


def test_features_to_matrix_and_group_split():
    feats = train_ref.rare_class_features()
    X, y = audioTrainTest.features_to_matrix(feats)
    Xr, yr = train_ref.features_to_matrix(feats)
    assert np.array_equal(X, Xr) and np.array_equal(y, yr) and y.dtype == np.float64
    one, lab = audioTrainTest.features_to_matrix(feats[:1])
    assert one is feats[0] and lab.shape == (25, 1) and not lab.any()
    assert [a.size for a in audioTrainTest.features_to_matrix([])] == [0, 0]
    tr, te = [np.array([3, 1]), np.array([0])], [np.array([2]), np.array([46, 5])]
    a, b, c, d = audioTrainTest.group_split(X, y, tr, te, 1)
    assert np.array_equal(a, X[[0]]) and np.array_equal(b, X[[46, 5]]) and np.array_equal(c, y[[0]]) and np.array_equal(d, y[[46, 5]])
    knn = audioTrainTest.train_knn(X, y, 3)
    assert isinstance(knn, audioTrainTest.Knn) and knn.features is X and knn.labels is y and knn.neighbors == 3


class _Call:
    """A valid two-job call of paa_knn_splits_f64 whose arguments can be replaced one at a time."""

    def __init__(self):
        self.n_samples, self.n_dims, self.n_jobs, self.max_classes = 6, 3, 2, 2
        self.X = np.zeros((6, 3))
        self.labels = np.array([0, 1, 0, 1, 0, 1], dtype=np.int32)
        self.train_off, self.train_idx = np.array([0, 3, 5], dtype=np.int64), np.array([0, 1, 2, 3, 4], dtype=np.int32)
        self.test_off, self.test_idx = np.array([0, 2, 3], dtype=np.int64), np.array([4, 5, 0], dtype=np.int32)
        self.mean, self.std = np.zeros((2, 3)), np.ones((2, 3))
        self.k, self.n_classes = np.array([1, 2], dtype=np.int32), np.array([2, 2], dtype=np.int32)
        self.label_out, self.proba_out, self.neighbors_out = np.zeros(3, dtype=np.int32), np.zeros((3, 2)), np.zeros((3, 2), dtype=np.int32)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)

        def p(a, kind):
            return None if a is None else a.ctypes.data_as(kind)
        return _ffi.lib().paa_knn_splits_f64(
            p(self.X, _ffi.c_f64p), self.n_samples, self.n_dims, p(self.labels, _ffi.c_i32p), self.n_jobs, p(self.train_off, _ffi.c_i64p),
            p(self.train_idx, _ffi.c_i32p), p(self.test_off, _ffi.c_i64p), p(self.test_idx, _ffi.c_i32p), p(self.mean, _ffi.c_f64p),
            p(self.std, _ffi.c_f64p), p(self.k, _ffi.c_i32p), p(self.n_classes, _ffi.c_i32p), self.max_classes,
            p(self.label_out, _ffi.c_i32p), p(self.proba_out, _ffi.c_f64p), p(self.neighbors_out, _ffi.c_i32p))


def _i32(*v):
    return np.array(v, dtype=np.int32)


def _i64(*v):
    return np.array(v, dtype=np.int64)


def test_c_abi_rejects_bad_split_jobs_before_any_device_work():
    """PAA_ERR_ARG with a message for every argument error of paa_knn_splits_f64; the same value with and without a GPU,
    because the arguments are judged before the device is initialised (on a host without one any later return would be the
    no-device error)."""
    for name in ("X", "labels", "train_off", "train_idx", "test_off", "test_idx", "mean", "std", "k", "n_classes", "label_out"):
        assert _Call()(**{name: None}) == _ffi.ERR_ARG, name
    bad = [dict(train_off=_i64(0, 3, 2)), dict(test_off=_i64(0, 2, 1)), dict(train_off=_i64(1, 3, 5)), dict(test_off=_i64(-1, 2, 3)),
           dict(train_idx=_i32(0, 1, 2, 3, 6)), dict(train_idx=_i32(0, -1, 2, 3, 4)), dict(test_idx=_i32(4, 6, 0)),
           dict(test_idx=_i32(-1, 5, 0)), dict(k=_i32(0, 2)), dict(k=_i32(1, 33)), dict(n_classes=_i32(0, 2)), dict(n_classes=_i32(2, 3)),
           dict(max_classes=65, n_classes=_i32(2, 65)), dict(max_classes=0), dict(n_dims=0), dict(n_dims=257), dict(n_jobs=0),
           dict(n_samples=0), dict(n_samples=2**31), dict(train_off=_i64(0, 0, 5)),        # an empty train list
           dict(test_off=_i64(0, 2, 2**31))]                                                # Q beyond the grid limit: judged from the offsets
    for kw in bad:
        assert _Call()(**kw) == _ffi.ERR_ARG, kw
        assert _ffi.last_error()
    # every test list empty: legal, nothing to do, no device needed
    call = _Call()
    call.label_out[:] = 7
    assert call(test_off=_i64(0, 0, 0)) == _ffi.PAA_OK and np.all(call.label_out == 7)
    geo = np.zeros(10, dtype=np.int32)
    assert _ffi.lib().paa_debug_knn_split_geometry(geo.ctypes.data_as(_ffi.c_i32p)) == _ffi.PAA_OK
    assert geo[:4].tolist() == [16, 16, 8, 6] and geo[4:].tolist() == [1, 2, 4, 8, 16, 32]
    assert _ffi.lib().paa_debug_knn_split_geometry(None) == _ffi.ERR_ARG
    assert audioTrainTest.knn_split_geometry() == (16, 16, 8, (1, 2, 4, 8, 16, 32))


def test_python_entry_points_reject_bad_shapes():
    X = np.zeros((6, 3))
    y = np.array([0., 1, 0, 1, 0, 1])
    job = (np.array([0, 1, 2]), np.array([3, 4]), np.zeros(3), np.ones(3), 1)
    bad = [(np.zeros(6), y, [job]), (X, y[:5], [job]), (X, y, []), (X, y, [job[:4]]), (X, y, [(job[0], job[1], np.zeros(2), np.ones(3), 1)]),
           (X, y, [(job[0], job[1], np.zeros(3), np.ones(4), 1)]), (X, y, [(np.array([[0, 1]]), job[1], job[2], job[3], 1)]),
           (X, y, [(np.array([0.5, 1.0]), job[1], job[2], job[3], 1)]), (X, y, [(job[0], np.array([2**31]), job[2], job[3], 1)]),
           (np.zeros((0, 3)), y[:0], [job])]
    for args in bad:
        with pytest.raises(ValueError):
            audioTrainTest.knn_split_predict(*args)
    # what the library judges (index range, k, an empty train list) arrives as its argument error
    for j in ((job[0], np.array([6]), job[2], job[3], 1), (job[0], job[1], job[2], job[3], 33), (np.array([], dtype=np.int64), job[1], job[2], job[3], 1)):
        with pytest.raises(ValueError):
            audioTrainTest.knn_split_predict(X, y, [j])
    feats = train_ref.three_class_features()
    with pytest.raises(NotImplementedError):
        audioTrainTest.evaluate_classifier(feats, ["a", "b", "c"], "knn", [1], 0, smote=True)
    with pytest.raises(NotImplementedError):
        audioTrainTest.extract_features_and_train(["x"], 1.0, 1.0, 0.05, 0.05, "knn", "model", use_smote=True)
    with pytest.raises(NotImplementedError):
        audioTrainTest.evaluate_classifier(feats, ["a", "b", "c"], "bayes", [1], 0)
    with pytest.raises(ValueError):
        audioTrainTest.evaluate_classifier(feats, ["a", "b"], "knn", [1], 0)


def test_evaluate_classifier_has_no_cpu_fallback():
    pytest.importorskip("sklearn")
    if _ffi.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_ffi.HipLibraryError):
        audioTrainTest.evaluate_classifier(train_ref.three_class_features(), ["a", "b", "c"], "knn", [1, 3], 0, n_exp=1)
