"""CPU-side checks of the GPU gradient-boosting fit (K20): the NumPy restatement (tests/boost_ref.py) against the goldens
(scripts/make_boost_golden.py: live scikit-learn 1.7.2) and against live scikit-learn -- equality where the sums are exact, the 1e-9
gate elsewhere --, the init bits, the replayed RandomState stream, to_sklearn_boosting, and the refusals of the Python keywords and
of paa_tree_fit_boost_tasks_f64 / paa_boost_fit_splits_f64, which are reported before any device work.  No GPU needed."""
import ctypes as C
import hashlib
import inspect
import os
import pickle

import numpy as np
import pytest

import boost_ref as B
from conftest import ROOT
from pyaudioanalysis_amd import _ffi, audioTrainTest as aT
from test_treefit_cpu import _i32, _i64, _p, golden, needs_no_device

FIELDS = B.FIELDS
GATE = 1e-9


def live_sklearn():
    sklearn = pytest.importorskip("sklearn")
    want = str(golden("boost_builder.npz")["sklearn_version"])
    if sklearn.__version__ != want:
        pytest.skip("the fit restates scikit-learn %s; %s is installed" % (want, sklearn.__version__))
    return sklearn


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), np.finfo(np.float64).tiny))) if a.size else 0.0


def same_tree(got, g, prefix, what):
    for f in FIELDS:
        a, b = np.asarray(got[f]), g[prefix + f]
        assert a.shape == b.shape, (what, f, a.shape, b.shape)
        if b.dtype.kind == "f":
            assert a.dtype == np.float64 and np.array_equal(a.view(np.int64), b.view(np.int64)), (what, f)      # bit for bit
        else:
            assert np.array_equal(a, b), (what, f)


def _digest(case):
    h = hashlib.sha256()
    for name in ("X", "y", "w", "mean", "scale"):
        h.update(np.ascontiguousarray(case[name]).tobytes())
    return h.hexdigest()


def builder_golden():
    """(the builder's cases with the row limit last, their golden): the inputs are regenerated and checked against the recorded digests."""
    g = golden("boost_builder.npz")
    cases = dict(B.builder_cases(), row_limit=B.limit_case())
    assert list(g["names"]) == list(cases)
    for i, c in enumerate(cases.values()):
        assert str(g["c%d_digest" % i]) == _digest(c), i
    return cases, g


def stage0_golden(name):
    g = golden("boost_stage0.npz")
    p = "s%d_" % list(g["names"]).index(name)
    X, y, K, rs = B.stage0_case(name)
    assert np.array_equal(g[p + "X"].astype(np.float64), X) and np.array_equal(g[p + "y"], y) and (int(g[p + "K"]), int(g[p + "random_state"])) == (K, rs)
    return g, p, X, y, K, rs


def whole_golden(name):
    g = golden("boost_whole.npz")
    p = "w%d_" % list(g["names"]).index(name)
    X, y, tr, te, K, stages, rs = B.whole_case(name)
    assert np.array_equal(g[p + "X"].astype(np.float64), X) and np.array_equal(g[p + "y"], y) and np.array_equal(g[p + "train"], tr)
    assert (int(g[p + "K"]), int(g[p + "n_stages"]), int(g[p + "random_state"])) == (K, stages, rs)
    return g, p, X, y, tr, te, K, stages, rs


def test_builder_restatement_equals_the_goldens():
    cases, g = builder_golden()
    for i, (name, c) in enumerate(cases.items()):
        same_tree(B.fit_tree(B.standardize32(c["X"], c["mean"], c["scale"]), c["y"], c["w"], c["seed"], c["max_depth"]), g, "c%d_" % i, name)
    at = lambda name, f: g["c%d_%s" % (list(cases).index(name), f)]        # noqa: E731
    assert [at("depth_%d" % d, "feature").shape[0] for d in (1, 2, 3)] == [3, 7, 15] and at("depth_12", "feature").shape[0] > 100
    assert at("one_row", "feature").tolist() == [-2] and at("constant_target", "feature").tolist() == [-2] and at("all_constant", "feature").tolist() == [-2]
    assert at("impure_at_the_limit", "impurity")[-1] > 1.0


@pytest.mark.parametrize("name", list(B.STAGE0))
def test_stage_0_restatement_equals_the_goldens_and_the_stream_replays(name):
    g, p, X, y, K, rs = stage0_golden(name)
    k_out = 1 if K == 2 else K
    assert B.tree_seeds(rs, k_out) == g[p + "seeds"].tolist() == aT.boosting_tree_seeds(rs, k_out)
    trees, score, raw, init = B.fit(X, y, K, 1, g[p + "seeds"].tolist())
    assert np.array_equal(init, g[p + "init"]) and np.array_equal(raw, g[p + "train_raw"]) and rel(score, g[p + "train_score"]) <= GATE
    for t, tree in enumerate(trees):
        lo, hi = int(g[p + "node_offsets"][t]), int(g[p + "node_offsets"][t + 1])
        for f in FIELDS:
            want = g[p + f][lo:hi]
            assert np.asarray(tree[f]).reshape(-1).astype(want.dtype).tobytes() == want.tobytes(), (name, t, f)
    assert np.array_equal(aT.boosting_init(y, K), g[p + "init"])


@pytest.mark.parametrize("name", list(B.WHOLE))
def test_whole_fit_restatement_is_within_the_gate(name):
    g, p, X, y, tr, te, K, stages, rs = whole_golden(name)
    trees, score, raw, init = B.fit(X[tr], y[tr], K, stages, g[p + "seeds"].tolist())
    assert np.array_equal(init, g[p + "init"])
    assert rel(score, g[p + "train_score"]) <= GATE and rel(raw, g[p + "train_raw"]) <= GATE
    k_out = 1 if K == 2 else K
    resid = B.gradient_and_loss(np.tile(init, (len(tr), 1)), y[tr], K)[0]
    for k in range(k_out):                                                          # the exact-arithmetic walk, on the stage-0 trees
        B.check_boost_stage(trees[k], X[tr].astype(np.float32), resid[:, k], np.ones(len(tr), dtype=int), B.MAX_DEPTH)


def test_restatement_against_live_scikit_learn():
    live_sklearn()
    for name in B.STAGE0:
        g, p, X, y, K, rs = stage0_golden(name)
        m = B.sklearn_fit(X, y, 1, rs)
        assert np.array_equal(m.train_score_, g[p + "train_score"]) and np.array_equal(m._raw_predict(X.astype(np.float32)), g[p + "train_raw"])
        # the replayed stream: the seeds, handed to single regressors on the stage-0 residuals, reproduce estimators_[0, k]
        resid = B.gradient_and_loss(np.tile(g[p + "init"], (len(y), 1)), y, K)[0]
        for k, seed in enumerate(g[p + "seeds"].tolist()):
            alone = B.sklearn_tree(X, resid[:, k], np.ones(len(y)), B.FixedSeed(seed), B.MAX_DEPTH)
            live = B.tree_arrays(m.estimators_[0, k].tree_)
            for f in ("children_left", "children_right", "feature", "threshold", "n_node_samples"):
                assert np.array_equal(alone[f], live[f]), (name, k, f)
    for name in B.WHOLE:
        g, p, X, y, tr, te, K, stages, rs = whole_golden(name)
        m = B.sklearn_fit(X[tr], y[tr], stages, rs)
        assert np.array_equal(m.train_score_, g[p + "train_score"]) and np.array_equal(m.predict_proba(X[te].astype(np.float32)), g[p + "test_proba"])


def test_init_bits_equal_a_live_fit():
    live_sklearn()
    from sklearn.ensemble import GradientBoostingClassifier
    for K in (2, 3, 4, 8):
        for balanced in (True, False):
            X, y = B._classes_case(5, 80, 3, K, balanced)
            m = GradientBoostingClassifier(n_estimators=1, random_state=0).fit(X.astype(np.float32), y)
            live = m._raw_predict_init(X[:1].astype(np.float32))[0]
            assert np.array_equal(B.init_raw(y, K)[:len(live)], live) and np.array_equal(aT.boosting_init(y, K), live), (K, balanced)
    assert aT.boosting_init(np.arange(80) % 8, 8)[0] != 0.0                        # -2.2e-16, carried as it is


def test_to_sklearn_boosting_round_trip():
    sklearn = live_sklearn()
    import sklearn.ensemble
    for name in ("fit_2x150x5", "fit_3x150x9_unbalanced"):
        X, y, tr, te, K, stages, rs = B.whole_case(name)
        m = B.sklearn_fit(X[tr], y[tr], stages, rs)
        arrays = aT.forest_arrays(m)
        assert arrays.kind == "boosted"
        arrays.train_score_ = m.train_score_
        back = aT.to_sklearn_boosting(arrays)
        assert type(back) is sklearn.ensemble.GradientBoostingClassifier and back.estimators_.shape == m.estimators_.shape
        assert back.n_trees_per_iteration_ == m.n_trees_per_iteration_ and np.array_equal(back.classes_, m.classes_)
        Z = X[te].astype(np.float32)
        again = pickle.loads(pickle.dumps(back))
        for b in (back, again):
            assert np.array_equal(b.predict_proba(Z), m.predict_proba(Z)) and np.array_equal(b.predict(Z), m.predict(Z))
            assert np.array_equal(b._raw_predict_init(Z), m._raw_predict_init(Z)) and np.array_equal(b.train_score_, m.train_score_)
        assert type(back.estimators_[0, 0]).__name__ == "DecisionTreeRegressor" and aT.is_forest(back)
    with pytest.raises(ValueError, match="boosted"):
        aT.to_sklearn_boosting(aT.forest_arrays(sklearn.ensemble.RandomForestClassifier(n_estimators=2).fit(X, y)))


def test_python_refusals_come_before_any_device_work():
    for fn in (aT.evaluate_classifier, aT.evaluate_classifier_full, aT.extract_features_and_train):
        assert inspect.signature(fn).parameters["boosting_fit"].kind is inspect.Parameter.KEYWORD_ONLY
        assert inspect.signature(fn).parameters["boosting_fit"].default == "sklearn"
    with pytest.raises(TypeError):
        aT.evaluate_classifier(None, None, "gradientboosting", [2], 0, None, 2, 0.9, False, "sklearn", "sklearn", "device")
    for kind in ("svm", "svm_rbf", "knn", "randomforest", "extratrees"):
        with pytest.raises(ValueError, match="boosting_fit"):
            aT.evaluate_classifier(None, None, kind, [2], 0, boosting_fit="device")
        with pytest.raises(ValueError, match="boosting_fit"):
            aT.extract_features_and_train(["/nonexistent"], 1.0, 1.0, 0.05, 0.05, kind, "m", boosting_fit="device")
    for bad in ("gpu", 1, None, True):
        with pytest.raises(ValueError, match="boosting_fit"):
            aT.evaluate_classifier(None, None, "gradientboosting", [2], 0, boosting_fit=bad)
        with pytest.raises(ValueError, match="boosting_fit"):
            aT.extract_features_and_train(["/nonexistent"], 1.0, 1.0, 0.05, 0.05, "gradientboosting", "m", boosting_fit=bad)
    with pytest.raises(ValueError, match="forest_fit"):                             # the pin of the forest keyword stays
        aT.evaluate_classifier(None, None, "gradientboosting", [2], 0, forest_fit="device")
    with pytest.raises(NotImplementedError, match="smote"):
        aT.evaluate_classifier(None, None, "gradientboosting", [2], 0, smote=True, boosting_fit="device")
    with pytest.raises(NotImplementedError, match="smote"):
        aT.extract_features_and_train(["/nonexistent"], 1.0, 1.0, 0.05, 0.05, "gradientboosting", "m", use_smote=True, boosting_fit="device")
    # the row limit and a one-class job: refused in Python, before the library is asked
    n = aT.TREE_MAX_ROWS + 1
    big = np.zeros((n, 2))
    with pytest.raises(NotImplementedError, match="8192"):
        aT.boosting_split_fit_predict(big, np.arange(n) % 2, [(np.arange(n), np.arange(2), np.zeros(2), np.ones(2), (1, 0))])
    with pytest.raises(NotImplementedError, match="8192"):
        aT.train_gradient_boosting_device(big, np.arange(n) % 2, 3, random_state=0)
    with pytest.raises(NotImplementedError, match="8192"):
        aT.tree_fit_boosting(big, [(np.arange(n), np.zeros(n), None, 1, np.zeros(2), np.ones(2))])
    X, y = np.zeros((6, 3)), np.array([0, 1, 0, 1, 2, 2])
    job = (np.arange(4), np.arange(4, 6), np.zeros(3), np.ones(3), (2, 1))
    with pytest.raises(ValueError, match="minimum of 2 classes"):
        aT.boosting_split_fit_predict(X, np.zeros(6, dtype=int), [job])
    with pytest.raises(ValueError, match="minimum of 2 classes"):
        aT.train_gradient_boosting_device(X, np.ones(6), 3)
    # malformed jobs and tasks
    for args in ((np.zeros(6), y, [job]), (X, y[:5], [job]), (X, y, []), (X, y, [job[:4]])):
        with pytest.raises(ValueError):
            aT.boosting_split_fit_predict(*args)
    with pytest.raises(ValueError):
        aT.boosting_split_fit_predict(X, y, [job[:4] + ((0, 1),)])
    t = np.arange(6) / 8
    task = lambda: (np.arange(6), t, None, 7, np.zeros(3), np.ones(3))          # noqa: E731
    for tasks in ([], [task()[:5]], [(np.arange(6), t[:2]) + task()[2:]], [task()[:3] + (-1,) + task()[4:]]):
        with pytest.raises(ValueError):
            aT.tree_fit_boosting(X, tasks)
    for depth in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="max_depth"):
            aT.tree_fit_boosting(X, [task()], max_depth=depth)
    bad = t.copy()
    bad[1] = np.nan
    with pytest.raises(ValueError, match="Input y contains NaN."):
        aT.tree_fit_boosting(X, [(np.arange(6), bad, None, 7, np.zeros(3), np.ones(3))])
    for args in ((np.zeros(6), y, 3), (X, y[:5], 3), (X, y, 0)):
        with pytest.raises(ValueError):
            aT.train_gradient_boosting_device(*args)
    # the pins of the forest entry points stay
    for call in (lambda: aT.forest_split_fit_predict(X, y, [job], "gradientboosting"), lambda: aT.train_forest_device(X, y, 2, "gradientboosting")):
        with pytest.raises(ValueError):
            call()


class _Tasks:
    """A valid call of paa_tree_fit_boost_tasks_f64 (two jobs, three trees) whose arguments can be replaced one at a time."""

    def __init__(self):
        self.n_samples, self.n_dims, self.n_jobs, self.n_tasks, self.max_depth = 6, 3, 2, 3, 3
        self.X = np.zeros((6, 3))
        self.job_off, self.job_idx, self.job_target = _i64(0, 3, 5), _i32(0, 1, 2, 3, 4), np.array([0.5, -1.0, 2.0, 0.0, 1.125])
        self.mean, self.std = np.zeros((2, 3)), np.ones((2, 3))
        self.task_job, self.task_seed, self.task_weight = _i32(0, 1, 0), _i64(1, 2, 3), _i32(1, 1, 1, 2, 0, 0, 1, 1)
        self.total_nodes, self.total_values = 5 + 1 + 3, 5 + 1 + 3
        self.job_flags, self.node_count = np.zeros(2, dtype=np.int32), np.zeros(3, dtype=np.int32)
        for name in ("children_left", "children_right", "feature", "n_node_samples"):
            setattr(self, name, np.zeros(9, dtype=np.int32))
        for name in ("threshold", "impurity", "weighted", "value"):
            setattr(self, name, np.zeros(9))
        self.missing = np.zeros(9, dtype=np.uint8)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        return _ffi.lib().paa_tree_fit_boost_tasks_f64(
            _p(self.X, _ffi.c_f64p), self.n_samples, self.n_dims, self.n_jobs, _p(self.job_off, _ffi.c_i64p), _p(self.job_idx, _ffi.c_i32p),
            _p(self.job_target, _ffi.c_f64p), _p(self.mean, _ffi.c_f64p), _p(self.std, _ffi.c_f64p), self.n_tasks,
            _p(self.task_job, _ffi.c_i32p), _p(self.task_seed, _ffi.c_i64p), _p(self.task_weight, _ffi.c_i32p), self.max_depth, self.total_nodes,
            self.total_values, _p(self.job_flags, _ffi.c_i32p), _p(self.node_count, _ffi.c_i32p), _p(self.children_left, _ffi.c_i32p),
            _p(self.children_right, _ffi.c_i32p), _p(self.feature, _ffi.c_i32p), _p(self.threshold, _ffi.c_f64p), _p(self.impurity, _ffi.c_f64p),
            _p(self.n_node_samples, _ffi.c_i32p), _p(self.weighted, _ffi.c_f64p), _p(self.missing, C.POINTER(C.c_uint8)), _p(self.value, _ffi.c_f64p))


class _Splits:
    """A valid two-job call of paa_boost_fit_splits_f64 (3 and 2 classes; 2 and 1 stages) whose arguments can be replaced one at a time."""

    def __init__(self):
        self.n_samples, self.n_dims, self.n_jobs = 7, 3, 2
        self.X = np.zeros((7, 3))
        self.labels = _i32(0, 1, 2, 1, 4, 4, 1)
        self.train_off, self.train_idx = _i64(0, 4, 7), _i32(0, 1, 2, 3, 4, 5, 6)
        self.test_off, self.test_idx = _i64(0, 2, 3), _i32(4, 5, 0)
        self.mean, self.std = np.zeros((2, 3)), np.ones((2, 3))
        self.n_estimators, self.tree_seed = _i32(2, 1), _i64(1, 2, 3, 4, 5, 6, 7)
        self.init, self.max_classes, self.learning_rate, self.max_depth, self.chunk_bytes = np.zeros((2, 3)), 3, 0.1, 3, 0
        self.label_out, self.proba, self.train_score, self.train_raw = np.zeros(3, dtype=np.int32), np.zeros((3, 3)), np.zeros(3), np.zeros(4 * 3 + 3)
        self.train_resid = np.zeros(4 * 3 + 3)
        self.total_nodes, self.node_count = 0, None
        self.job_flags, self.n_chunks = np.zeros(2, dtype=np.int32), np.zeros(1, dtype=np.int32)

    def with_trees(self):
        self.total_nodes, self.node_count = 6 * 7 + 5, np.zeros(7, dtype=np.int32)
        return self

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        n = max(self.total_nodes, 1)
        i32, f64 = (lambda: np.zeros(n, dtype=np.int32)), (lambda: np.zeros(n))
        trees = self.total_nodes > 0
        arr = lambda a, t: _p(a, t) if trees else None                       # noqa: E731
        return _ffi.lib().paa_boost_fit_splits_f64(
            _p(self.X, _ffi.c_f64p), self.n_samples, self.n_dims, _p(self.labels, _ffi.c_i32p), self.n_jobs, _p(self.train_off, _ffi.c_i64p),
            _p(self.train_idx, _ffi.c_i32p), _p(self.test_off, _ffi.c_i64p), _p(self.test_idx, _ffi.c_i32p), _p(self.mean, _ffi.c_f64p),
            _p(self.std, _ffi.c_f64p), _p(self.n_estimators, _ffi.c_i32p), _p(self.tree_seed, _ffi.c_i64p), _p(self.init, _ffi.c_f64p),
            self.max_classes, self.learning_rate, self.max_depth, self.chunk_bytes, _p(self.label_out, _ffi.c_i32p), _p(self.proba, _ffi.c_f64p),
            _p(self.train_score, _ffi.c_f64p), _p(self.train_raw, _ffi.c_f64p), _p(self.train_resid, _ffi.c_f64p), self.total_nodes, _p(self.node_count, _ffi.c_i32p),
            arr(i32(), _ffi.c_i32p), arr(i32(), _ffi.c_i32p), arr(i32(), _ffi.c_i32p), arr(f64(), _ffi.c_f64p), arr(f64(), _ffi.c_f64p),
            arr(i32(), _ffi.c_i32p), arr(f64(), _ffi.c_f64p), arr(np.zeros(n, dtype=np.uint8), C.POINTER(C.c_uint8)), arr(f64(), _ffi.c_f64p),
            _p(self.job_flags, _ffi.c_i32p), _p(self.n_chunks, _ffi.c_i32p))


def test_c_abi_rejects_bad_boosting_tree_tasks_before_any_device_work():
    for name in ("X", "job_off", "job_idx", "job_target", "mean", "std", "task_job", "task_seed", "task_weight", "job_flags", "node_count",
                 "children_left", "children_right", "feature", "threshold", "impurity", "n_node_samples", "weighted", "missing", "value"):
        assert _Tasks()(**{name: None}) == _ffi.ERR_ARG, name
    target = lambda v: np.array([0.5, -1.0, v, 0.0, 1.125])          # noqa: E731
    bad = [dict(max_depth=0), dict(max_depth=-3), dict(max_depth=8193), dict(job_off=_i64(1, 3, 5)), dict(job_idx=_i32(0, 1, 2, 3, 6)),
           dict(job_target=target(np.nan)), dict(job_target=target(np.inf)), dict(n_dims=0), dict(n_tasks=0), dict(n_jobs=0), dict(n_samples=0),
           dict(task_job=_i32(0, 2, 0)), dict(task_seed=_i64(1, -1, 3)), dict(task_seed=_i64(1, 2**32, 3)),
           dict(task_weight=_i32(1, 1, 1, 0, 0, 0, 1, 1)), dict(task_weight=_i32(1, 8192, 1, 2, 0, 0, 1, 1)), dict(total_nodes=10), dict(total_values=18)]
    for kw in bad:
        assert _Tasks()(**kw) == _ffi.ERR_ARG, kw
        assert _ffi.last_error()
    assert _Tasks()(n_dims=257) == _ffi.ERR_UNSUPPORTED and "256" in _ffi.last_error()
    n = aT.TREE_MAX_ROWS + 1
    assert _Tasks()(n_jobs=1, n_tasks=1, job_off=_i64(0, n), job_idx=np.zeros(n, dtype=np.int32), job_target=np.zeros(n),
                    task_weight=np.ones(n, dtype=np.int32)) == _ffi.ERR_UNSUPPORTED
    assert "8192" in _ffi.last_error()
    assert aT.tree_fit_geometry() == (256, aT.TREE_MAX_ROWS, 64, 256, aT.TREE_MAX_WEIGHT, 1024)          # untouched


def test_c_abi_rejects_bad_boosting_split_jobs_before_any_device_work():
    for name in ("X", "labels", "train_off", "train_idx", "test_off", "test_idx", "mean", "std", "n_estimators", "tree_seed", "init", "label_out",
                 "job_flags"):
        assert _Splits()(**{name: None}) == _ffi.ERR_ARG, name
    assert _Splits().with_trees()(node_count=None) == _ffi.ERR_ARG
    bad = [dict(train_off=_i64(1, 4, 7)), dict(test_off=_i64(-1, 2, 3)), dict(train_off=_i64(0, 5, 4)), dict(train_idx=_i32(0, 1, 2, 3, 4, 5, 7)),
           dict(train_idx=_i32(0, -1, 2, 3, 4, 5, 6)), dict(test_idx=_i32(4, 7, 0)), dict(n_dims=0), dict(n_jobs=0), dict(n_samples=0),
           dict(labels=_i32(0, -1, 2, 1, 4, 4, 1)), dict(train_off=_i64(0, 0, 7)), dict(n_estimators=_i32(2, 0)), dict(tree_seed=_i64(1, 2, 3, 4, 5, 6, -7)),
           dict(labels=_i32(0, 1, 2, 1, 4, 4, 4)),                                 # job 1 holds one class
           dict(max_classes=2), dict(max_classes=1), dict(max_depth=0), dict(max_depth=21), dict(learning_rate=0.0), dict(learning_rate=np.nan),
           dict(init=np.full((2, 3), np.inf)), dict(test_off=_i64(0, 2, 2**31))]
    for kw in bad:
        assert _Splits()(**kw) == _ffi.ERR_ARG, kw
        assert _ffi.last_error()
    assert _Splits().with_trees()(total_nodes=46) == _ffi.ERR_ARG
    assert _Splits()(n_dims=257) == _ffi.ERR_UNSUPPORTED and "256" in _ffi.last_error()
    assert _Splits()(max_classes=65) == _ffi.ERR_UNSUPPORTED and "64" in _ffi.last_error()
    n = aT.TREE_MAX_ROWS + 1
    assert _Splits()(n_samples=n, X=np.zeros((n, 3)), labels=(np.arange(n) % 2).astype(np.int32), n_jobs=1, train_off=_i64(0, n),
                     train_idx=np.arange(n, dtype=np.int32), test_off=_i64(0, 1), n_estimators=_i32(1)) == _ffi.ERR_UNSUPPORTED
    assert "8192" in _ffi.last_error()


@needs_no_device
def test_valid_calls_reach_the_device_and_fail_there():
    """The templates above are valid: without a device they pass every check and stop at the missing device."""
    assert _Tasks()() == _ffi.ERR_HIP and _Splits()() == _ffi.ERR_HIP and _Splits().with_trees()() == _ffi.ERR_HIP
    assert _Splits()(proba=None, train_score=None, train_raw=None, train_resid=None, n_chunks=None) == _ffi.ERR_HIP
    X, y, tr, te, K, stages, rs = B.whole_case("fit_2x150x5")
    with pytest.raises(_ffi.HipLibraryError):
        aT.train_gradient_boosting_device(X[tr], y[tr], 2, random_state=1)
    with pytest.raises(_ffi.HipLibraryError):
        aT.tree_fit_boosting(X, [(tr, y[tr].astype(float), None, 1, np.zeros(5), np.ones(5))])


def test_new_symbols_are_declared_bound_and_built():
    from pyaudioanalysis_amd import _build
    header = open(os.path.join(ROOT, "include", "paa_hip.h")).read()
    for s in ("paa_tree_fit_boost_tasks_f64", "paa_boost_fit_splits_f64"):
        assert s in _ffi.EXPORTED_SYMBOLS and hasattr(_ffi.lib(), s) and ("int %s(" % s) in header, s
    assert len(_build.SOURCES) == 18 and "kernels_boost.hpp" in _build.HEADERS and "lib_boost.hpp" in _build.HEADERS
    unit = open(os.path.join(ROOT, "pyaudioanalysis_amd", "csrc", "family_forest.hip")).read()
    assert '#include "kernels_boost.hpp"' in unit and "tree_fit_kernel<kBest, kFriedman>" in unit and "boost_gradient_kernel" in unit
    for name in ("tree_fit_boosting", "boosting_split_fit_predict", "train_gradient_boosting_device", "to_sklearn_boosting", "boosting_tree_seeds",
                 "boosting_init"):
        assert callable(getattr(aT, name)), name
