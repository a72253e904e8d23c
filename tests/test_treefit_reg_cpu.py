"""CPU-side checks of the GPU regression-tree builder (K19): the NumPy restatement (tests/treefit_reg_ref.py) against the goldens
(scripts/make_treefit_reg_golden.py: scikit-learn 1.7.2's own trees) and against live scikit-learn, the exactness premise that lets
the goldens demand equality, the exact-arithmetic walk that general targets are held to, to_sklearn_forest_regressor, and the
argument errors of paa_tree_fit_reg_tasks_f64 / paa_forest_reg_fit_splits_f64 and of the Python keywords, which are reported before
any device work.  No GPU needed."""
import ctypes as C
import inspect
import os
import pickle

import numpy as np
import pytest

import treefit_reg_ref as R
from conftest import ROOT
from pyaudioanalysis_amd import _ffi, audioTrainTest as aT
from test_treefit_cpu import _i32, _i64, _p, golden, golden_case, needs_no_device

FIELDS = R.FIELDS


def live_sklearn():
    """scikit-learn, when it is installed in the version the builder restates and the goldens record; otherwise the test skips."""
    sklearn = pytest.importorskip("sklearn")
    want = str(golden("treefit_reg_edges.npz")["sklearn_version"])
    if sklearn.__version__ != want:
        pytest.skip("the builder restates scikit-learn %s; %s is installed" % (want, sklearn.__version__))
    return sklearn


def same_tree(got, g, prefix, what):
    for f in FIELDS:
        a, b = np.asarray(got[f]), g[prefix + f]
        assert a.shape == b.shape, (what, f, a.shape, b.shape)
        if b.dtype.kind == "f":
            assert a.dtype == np.float64 and np.array_equal(a.view(np.int64), b.view(np.int64)), (what, f)      # bit for bit
        else:
            assert np.array_equal(a, b), (what, f)


def test_cases_in_the_tree_are_the_recorded_ones():
    g = golden("treefit_reg_edges.npz")
    cases = R.edge_cases()
    assert str(g["kind"]) == "treefit_reg" and list(g["names"]) == list(cases)
    for i, (name, case) in enumerate(cases.items()):
        R.assert_exact(case["y"], case["w"])
        for k, v in golden_case(g, i).items():
            assert np.array_equal(v, case[k]), (name, k)
    lim = R.limit_case()
    R.assert_exact(lim["y"], lim["w"])
    g = golden("treefit_reg_limit.npz")
    assert np.array_equal(g["c0_X"].astype(np.float64), lim["X"]) and np.array_equal(g["c0_y"], lim["y"]) and int(g["c0_seed"]) == lim["seed"]
    assert lim["X"].shape == (aT.TREE_MAX_ROWS, 4) and int(np.count_nonzero(lim["w"])) == aT.TREE_MAX_ROWS
    X, y, jobs = R.sweep_case()
    g = golden("treefit_reg_sweep.npz")
    assert np.array_equal(g["X"], X) and np.array_equal(g["y"], y) and int(g["n_jobs"]) == len(jobs) == 6
    for j, job in enumerate(jobs):
        assert np.array_equal(g["j%d_train" % j], job[0]) and np.array_equal(g["j%d_test" % j], job[1])
        assert (int(g["j%d_n_estimators" % j]), int(g["j%d_seed" % j])) == job[4]
    assert sorted(j[4][0] for j in jobs) == [1, 2, 3, 4, 5, 7] and [len(j[1]) for j in jobs].count(1) == 1


def test_restatement_equals_the_goldens():
    g = golden("treefit_reg_edges.npz")
    for i, name in enumerate(g["names"]):
        c = golden_case(g, i)
        same_tree(R.fit_tree(R.standardize32(c["X"], c["mean"], c["scale"]), c["y"], c["w"], c["seed"]), g, "c%d_" % i, name)
    # what the cases are there for
    names = list(g["names"])
    at = lambda name, f: g["c%d_%s" % (names.index(name), f)]        # noqa: E731
    assert at("one_in_bag_row", "feature").tolist() == [-2] and at("one_in_bag_row", "value").tolist() == [[-2.25]]
    assert at("two_rows_equal_targets", "feature").tolist() == [-2] and at("two_rows_equal_targets", "impurity").tolist() == [0.0]
    assert at("two_rows_distinct_targets", "feature").tolist() == [0, -2, -2] and at("two_rows_distinct_targets", "value").tolist() == [[-1.0625], [1.0], [-3.125]]
    assert at("all_constant", "feature").tolist() == [-2] and at("all_constant", "impurity")[0] > 0.1      # an impure leaf
    assert at("constant_target", "feature").tolist() == [-2] and at("constant_target", "value").tolist() == [[7.375]]
    assert set(at("three_of_five_constant", "feature").tolist()) == {-2, 1, 3}
    assert set(at("dims_1", "feature").tolist()) == {-2, 0} and at("dims_256_few_rows", "feature").max() > 9
    left, right = at("chain_300", "children_left"), at("chain_300", "children_right")
    assert left.shape == (599,) and np.all(left[right[left >= 0]] == -1)             # every right child a leaf: 299 pending at once
    assert np.abs(at("both_signs_at_the_bound", "value")).max() == 1024.0
    assert at("one_row_of_weight_8191", "weighted_n_node_samples").tolist() in ([8192.0, 1.0, 8191.0], [8192.0, 8191.0, 1.0])
    lim = golden("treefit_reg_limit.npz")
    assert lim["c0_n_node_samples"][0] == 8192 and lim["c0_feature"].shape[0] > 4000


def test_restatement_equals_the_row_limit_golden():
    g = golden("treefit_reg_limit.npz")
    c = golden_case(g, 0)
    same_tree(R.fit_tree(c["X"].astype(np.float32), c["y"], c["w"], c["seed"]), g, "c0_", "row limit")


def test_restatement_equals_live_scikit_learn():
    live_sklearn()
    for name, c in R.edge_cases().items():
        x32 = R.standardize32(c["X"], c["mean"], c["scale"])
        ref = R.sklearn_tree(x32, c["y"], c["w"], R.FixedSeed(c["seed"]))
        got = R.fit_tree(x32, c["y"], c["w"], c["seed"])
        for f in FIELDS:
            assert np.asarray(got[f]).shape == ref[f].shape and np.array_equal(got[f], ref[f]), (name, f)
    rng = np.random.default_rng(8)                                                  # and through an integer random_state
    X, y, w = rng.standard_normal((150, 9)), R.eighths(rng.standard_normal(150) * 9), R.bootstrap_weights(11, 150)
    ref = R.sklearn_tree(X.astype(np.float32), y, w, 11)
    got = R.fit_tree(X.astype(np.float32), y, w, R.splitter_seed(11))
    assert all(np.array_equal(got[f], ref[f]) for f in FIELDS)


def test_exact_targets_do_not_depend_on_the_order_of_the_rows():
    """The exactness premise: a golden case gives the same arrays after a permutation of its rows (every sum of the criterion is exact,
    so no order of summation can change a bit)."""
    g = golden("treefit_reg_edges.npz")
    i = list(g["names"]).index("bootstrap_260x9")
    c = golden_case(g, i)
    perm = np.random.default_rng(2).permutation(c["X"].shape[0])
    x32 = R.standardize32(c["X"], c["mean"], c["scale"])
    same_tree(R.fit_tree(x32[perm], c["y"][perm], c["w"][perm], c["seed"]), g, "c%d_" % i, "permuted rows")
    live_sklearn()
    ref = R.sklearn_tree(x32[perm], c["y"][perm], c["w"][perm], R.FixedSeed(c["seed"]))
    same_tree(ref, g, "c%d_" % i, "scikit-learn on permuted rows")


@pytest.mark.parametrize("bootstrap", [False, True])
def test_scikit_learns_own_trees_pass_the_walk_for_general_targets(bootstrap):
    """The input of the GPU test's general-target cases is chosen so that scikit-learn's own trees satisfy the derived bounds."""
    live_sklearn()
    X, y = R.general_case()
    w = R.bootstrap_weights(7, X.shape[0]) if bootstrap else np.ones(X.shape[0], dtype=np.int64)
    x32 = X.astype(np.float32)
    assert all(np.unique(x32[:, d]).shape[0] == X.shape[0] for d in range(X.shape[1])) and np.unique(y).shape[0] == X.shape[0]
    assert R.check_cart_tree(R.sklearn_tree(x32, y, w, 3), x32, y, w, distinct=not bootstrap) == int(np.count_nonzero(w)) - 1
    assert R.check_cart_tree(R.fit_tree(x32, y, w, 77), x32, y, w, distinct=not bootstrap) == int(np.count_nonzero(w)) - 1


def test_the_walk_refuses_a_wrong_tree():
    X, y = R.general_case(60, 3)
    x32, w = X.astype(np.float32), np.ones(60, dtype=np.int64)
    good = R.fit_tree(x32, y, w, 5)
    R.check_cart_tree(good, x32, y, w, distinct=True)
    for f, change in (("value", lambda a: a + 1e-9), ("threshold", lambda a: np.where(a != -2.0, a + 1e-3, a)),
                      ("weighted_n_node_samples", lambda a: a + 1.0)):
        with pytest.raises(AssertionError):
            R.check_cart_tree(dict(good, **{f: change(good[f])}), x32, y, w, distinct=True)
    worse = R.fit_tree(x32[:, :1], y, w, 5)                                         # a tree that never looked at two of the features
    with pytest.raises(AssertionError):
        R.check_cart_tree(worse, x32, y, w, distinct=True)


def test_to_sklearn_forest_regressor_predicts_and_pickles_like_the_model():
    sklearn = live_sklearn()
    import sklearn.ensemble
    X, y, jobs = R.sweep_case()
    m = sklearn.ensemble.RandomForestRegressor(n_estimators=6, random_state=4).fit(X, y)
    arrays = aT.forest_arrays(m)
    assert arrays.kind == "regressor"
    back = aT.to_sklearn_forest_regressor(arrays)
    assert type(back) is sklearn.ensemble.RandomForestRegressor and len(back.estimators_) == 6
    Z = np.random.default_rng(1).standard_normal((50, X.shape[1]))
    assert np.array_equal(back.predict(Z), m.predict(Z))
    again = pickle.loads(pickle.dumps(back))
    assert np.array_equal(again.predict(Z), m.predict(Z))
    for a, b in zip(back.estimators_, m.estimators_):
        assert a.tree_.max_depth == b.tree_.max_depth and a.tree_.node_count == b.tree_.node_count
    with pytest.raises(ValueError, match="regressor"):
        aT.to_sklearn_forest_regressor(aT.forest_arrays(sklearn.ensemble.RandomForestClassifier(n_estimators=2).fit(X, y > 0)))


def test_python_refusals_come_before_any_device_work():
    X, y = np.zeros((6, 3)), np.arange(6) / 8
    # the keyword: "randomforest" only, refused before any work; svm_fit keeps its own refusal
    assert list(inspect.signature(aT.evaluate_regression).parameters)[-2:] == ["svm_fit", "forest_fit"]
    assert inspect.signature(aT.evaluate_regression).parameters["forest_fit"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(aT.feature_extraction_train_regression).parameters["forest_fit"].kind is inspect.Parameter.KEYWORD_ONLY
    for method in ("svm", "svm_rbf"):
        with pytest.raises(ValueError, match="forest_fit"):
            aT.evaluate_regression(None, None, 2, method, [1.0], forest_fit="device")
        with pytest.raises(ValueError, match="forest_fit"):
            aT.feature_extraction_train_regression("/nonexistent", 1.0, 1.0, 0.05, 0.05, method, "m", forest_fit="device")
    with pytest.raises(ValueError, match="forest_fit"):
        aT.evaluate_regression(None, None, 2, "randomforest", [5], forest_fit="gpu")
    with pytest.raises(ValueError, match="svm_fit"):
        aT.evaluate_regression(None, None, 2, "randomforest", [5], svm_fit="device")
    with pytest.raises(NotImplementedError):
        aT.evaluate_regression(None, None, 2, "knn", [5], forest_fit="device")
    # targets: scikit-learn's messages
    job = (np.arange(4), np.arange(4, 6), np.zeros(3), np.ones(3), (2, 1))
    task = lambda t: (np.arange(6), t, None, 7, np.zeros(3), np.ones(3))          # noqa: E731
    for bad, text in ((np.nan, "Input y contains NaN."), (np.inf, "Input y contains infinity"), (-np.inf, "Input y contains infinity")):
        t = y.copy()
        t[2] = bad
        with pytest.raises(ValueError, match=text):
            aT.tree_fit_regression(X, [task(t)])
        with pytest.raises(ValueError, match=text):
            aT.forest_regression_split_fit_predict(X, t, [job])
        with pytest.raises(ValueError, match=text):
            aT.train_random_forest_regression_device(X, t, 3, random_state=0)
        with pytest.raises(ValueError, match=text):
            aT.evaluate_regression(np.random.default_rng(0).standard_normal((6, 3)), t, 2, "randomforest", [2], forest_fit="device")
    # the row limit: refused in Python, before the library is asked
    n = aT.TREE_MAX_ROWS + 1
    big, t = np.zeros((n, 2)), np.zeros(n)
    with pytest.raises(NotImplementedError, match="8192"):
        aT.tree_fit_regression(big, [(np.arange(n), t, None, 1, np.zeros(2), np.ones(2))])
    with pytest.raises(NotImplementedError, match="8192"):
        aT.train_random_forest_regression_device(big, t, 3, random_state=0)
    with pytest.raises(NotImplementedError, match="8192"):
        aT.forest_regression_split_fit_predict(big, t, [(np.arange(n), np.arange(2), np.zeros(2), np.ones(2), (1, 0))])
    with pytest.raises(NotImplementedError, match="8192"):
        aT.evaluate_regression(np.random.default_rng(0).standard_normal((9103, 2)), np.zeros(9103), 1, "randomforest", [2], forest_fit="device")
    # shapes and the library's argument errors
    for args in ((np.zeros(6), y, [job]), (X, y[:5], [job]), (X, y, []), (X, y, [job[:4]])):
        with pytest.raises(ValueError):
            aT.forest_regression_split_fit_predict(*args)
    with pytest.raises(ValueError):
        aT.forest_regression_split_fit_predict(X, y, [(job[0], job[1], job[2], job[3], (0, 1))])
    for tasks in ([], [task(y)[:5]], [(np.arange(6), y[:2]) + task(y)[2:]], [task(y)[:2] + (np.zeros(6, dtype=int),) + task(y)[3:]],
                  [task(y)[:3] + (-1,) + task(y)[4:]]):
        with pytest.raises(ValueError):
            aT.tree_fit_regression(X, tasks)
    for args in ((np.zeros(6), y, 3), (X, y[:5], 3), (X, y, 0)):
        with pytest.raises(ValueError):
            aT.train_random_forest_regression_device(*args)


class _Tasks:
    """A valid call of paa_tree_fit_reg_tasks_f64 (two jobs, three trees) whose arguments can be replaced one at a time."""

    def __init__(self):
        self.n_samples, self.n_dims, self.n_jobs, self.n_tasks = 6, 3, 2, 3
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
        return _ffi.lib().paa_tree_fit_reg_tasks_f64(
            _p(self.X, _ffi.c_f64p), self.n_samples, self.n_dims, self.n_jobs, _p(self.job_off, _ffi.c_i64p), _p(self.job_idx, _ffi.c_i32p),
            _p(self.job_target, _ffi.c_f64p), _p(self.mean, _ffi.c_f64p), _p(self.std, _ffi.c_f64p), self.n_tasks,
            _p(self.task_job, _ffi.c_i32p), _p(self.task_seed, _ffi.c_i64p), _p(self.task_weight, _ffi.c_i32p), self.total_nodes,
            self.total_values, _p(self.job_flags, _ffi.c_i32p), _p(self.node_count, _ffi.c_i32p), _p(self.children_left, _ffi.c_i32p),
            _p(self.children_right, _ffi.c_i32p), _p(self.feature, _ffi.c_i32p), _p(self.threshold, _ffi.c_f64p), _p(self.impurity, _ffi.c_f64p),
            _p(self.n_node_samples, _ffi.c_i32p), _p(self.weighted, _ffi.c_f64p), _p(self.missing, C.POINTER(C.c_uint8)), _p(self.value, _ffi.c_f64p))


class _Splits:
    """A valid two-job call of paa_forest_reg_fit_splits_f64 whose arguments can be replaced one at a time."""

    def __init__(self):
        self.n_samples, self.n_dims, self.n_jobs = 6, 3, 2
        self.X = np.zeros((6, 3))
        self.targets = np.array([0.5, -1.0, 2.0, 0.0, 1.125, 3.0])
        self.train_off, self.train_idx = _i64(0, 3, 6), _i32(0, 1, 2, 3, 4, 5)
        self.test_off, self.test_idx = _i64(0, 2, 3), _i32(4, 5, 0)
        self.mean, self.std = np.zeros((2, 3)), np.ones((2, 3))
        self.n_estimators, self.tree_seed, self.tree_weight = _i32(2, 1), _i64(1, 2, 3), _i32(1, 1, 1, 0, 2, 1, 3, 0, 0)
        self.pred, self.train_pred, self.job_flags = np.zeros(3), np.zeros(6), np.zeros(2, dtype=np.int32)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        return _ffi.lib().paa_forest_reg_fit_splits_f64(
            _p(self.X, _ffi.c_f64p), self.n_samples, self.n_dims, _p(self.targets, _ffi.c_f64p), self.n_jobs, _p(self.train_off, _ffi.c_i64p),
            _p(self.train_idx, _ffi.c_i32p), _p(self.test_off, _ffi.c_i64p), _p(self.test_idx, _ffi.c_i32p), _p(self.mean, _ffi.c_f64p),
            _p(self.std, _ffi.c_f64p), _p(self.n_estimators, _ffi.c_i32p), _p(self.tree_seed, _ffi.c_i64p),
            _p(self.tree_weight, _ffi.c_i32p), _p(self.pred, _ffi.c_f64p), _p(self.train_pred, _ffi.c_f64p), _p(self.job_flags, _ffi.c_i32p), None)


def test_c_abi_rejects_bad_regression_tree_tasks_before_any_device_work():
    names = ("X", "job_off", "job_idx", "job_target", "mean", "std", "task_job", "task_seed", "task_weight", "job_flags", "node_count",
             "children_left", "children_right", "feature", "threshold", "impurity", "n_node_samples", "weighted", "missing", "value")
    for name in names:
        assert _Tasks()(**{name: None}) == _ffi.ERR_ARG, name
    target = lambda v: np.array([0.5, -1.0, v, 0.0, 1.125])          # noqa: E731
    bad = [dict(job_off=_i64(1, 3, 5)), dict(job_off=_i64(0, 3, 2)), dict(job_off=_i64(0, 0, 5)), dict(job_idx=_i32(0, 1, 2, 3, 6)),
           dict(job_idx=_i32(0, -1, 2, 3, 4)), dict(job_target=target(np.nan)), dict(job_target=target(np.inf)), dict(job_target=target(-np.inf)),
           dict(n_dims=0), dict(n_tasks=0), dict(n_jobs=0), dict(n_samples=0), dict(n_samples=2**31),
           dict(task_job=_i32(0, 2, 0)), dict(task_job=_i32(0, -1, 0)), dict(task_seed=_i64(1, -1, 3)), dict(task_seed=_i64(1, 2**32, 3)),
           dict(task_weight=_i32(1, 1, 1, 0, 0, 0, 1, 1)),                       # tree 1: nothing in the bag
           dict(task_weight=_i32(1, -1, 1, 2, 0, 0, 1, 1)), dict(task_weight=_i32(1, 8192, 1, 2, 0, 0, 1, 1)),
           dict(total_nodes=10), dict(total_values=18)]                          # (one value per node)
    for kw in bad:
        assert _Tasks()(**kw) == _ffi.ERR_ARG, kw
        assert _ffi.last_error()
    # beyond the limits: refused with the limit in the message, no other path
    assert _Tasks()(n_dims=257) == _ffi.ERR_UNSUPPORTED and "256" in _ffi.last_error()
    n = aT.TREE_MAX_ROWS + 1
    assert _Tasks()(n_jobs=1, n_tasks=1, job_off=_i64(0, n), job_idx=np.zeros(n, dtype=np.int32), job_target=np.zeros(n),
                    task_weight=np.ones(n, dtype=np.int32)) == _ffi.ERR_UNSUPPORTED
    assert "8192" in _ffi.last_error()
    assert aT.tree_fit_geometry() == (256, aT.TREE_MAX_ROWS, 64, 256, aT.TREE_MAX_WEIGHT, 1024)          # untouched


def test_c_abi_rejects_bad_regression_split_jobs_before_any_device_work():
    for name in ("X", "targets", "train_off", "train_idx", "test_off", "test_idx", "mean", "std", "n_estimators", "tree_seed", "pred", "job_flags"):
        assert _Splits()(**{name: None}) == _ffi.ERR_ARG, name
    target = lambda v: np.array([0.5, -1.0, v, 0.0, 1.125, 3.0])          # noqa: E731
    bad = [dict(train_off=_i64(1, 3, 6)), dict(test_off=_i64(-1, 2, 3)), dict(train_off=_i64(0, 4, 3)), dict(test_off=_i64(0, 2, 1)),
           dict(train_idx=_i32(0, 1, 2, 3, 4, 6)), dict(train_idx=_i32(0, -1, 2, 3, 4, 5)), dict(test_idx=_i32(4, 6, 0)), dict(n_dims=0),
           dict(n_jobs=0), dict(n_samples=0), dict(targets=target(np.nan)), dict(targets=target(np.inf)), dict(train_off=_i64(0, 0, 6)),
           dict(n_estimators=_i32(2, 0)), dict(tree_seed=_i64(1, 2, -3)), dict(tree_weight=_i32(1, 1, 1, 0, 0, 0, 3, 0, 0)),
           dict(tree_weight=_i32(1, 1, 1, 0, 2, 1, 8192, 0, 0)), dict(test_off=_i64(0, 2, 2**31))]
    for kw in bad:
        assert _Splits()(**kw) == _ffi.ERR_ARG, kw
        assert _ffi.last_error()
    assert _Splits()(n_dims=257) == _ffi.ERR_UNSUPPORTED and "256" in _ffi.last_error()
    n = aT.TREE_MAX_ROWS + 1
    assert _Splits()(n_samples=n, X=np.zeros((n, 3)), targets=np.zeros(n), n_jobs=1, train_off=_i64(0, n), train_idx=np.arange(n, dtype=np.int32),
                     test_off=_i64(0, 1), n_estimators=_i32(1), tree_weight=None) == _ffi.ERR_UNSUPPORTED
    assert "8192" in _ffi.last_error()


@needs_no_device
def test_valid_calls_reach_the_device_and_fail_there():
    """The templates above are valid: without a device they pass every check and stop at the missing device."""
    assert _Tasks()() == _ffi.ERR_HIP and _Splits()() == _ffi.ERR_HIP and _Splits()(tree_weight=None, train_pred=None) == _ffi.ERR_HIP


def test_new_symbols_are_declared_bound_and_built():
    from pyaudioanalysis_amd import _build
    header = open(os.path.join(ROOT, "include", "paa_hip.h")).read()
    for s in ("paa_tree_fit_reg_tasks_f64", "paa_forest_reg_fit_splits_f64"):
        assert s in _ffi.EXPORTED_SYMBOLS and hasattr(_ffi.lib(), s) and ("int %s(" % s) in header, s
    assert len(_build.SOURCES) == 18 and "kernels_treefit.hpp" in _build.HEADERS and "lib_treefit.hpp" in _build.HEADERS
    for name in ("tree_fit_regression", "forest_regression_split_fit_predict", "train_random_forest_regression_device",
                 "to_sklearn_forest_regressor"):
        assert callable(getattr(aT, name)), name
