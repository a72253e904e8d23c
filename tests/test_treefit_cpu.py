"""CPU-side checks of the GPU tree builder: the NumPy restatement (tests/treefit_ref.py) against the goldens
(scripts/make_treefit_golden.py: scikit-learn 1.7.2's own trees) and against live scikit-learn, the host's seed and bootstrap
derivation against scikit-learn's forests, to_sklearn_forest, and the argument errors of paa_tree_fit_tasks_f64 /
paa_forest_fit_splits_f64 and of the Python keywords, which are reported before any device work.  Equality everywhere: integer
arrays equal, float64 arrays bit-equal.  No GPU needed."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

import train_ref
import treefit_ref as R
from conftest import ROOT
from pyaudioanalysis_amd import _ffi, audioTrainTest as aT

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIELDS = R.TREE_FIELDS + ("missing_go_to_left",)


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def live_sklearn():
    """scikit-learn, when it is installed in the version the builder restates and the goldens record; otherwise the test skips."""
    sklearn = pytest.importorskip("sklearn")
    want = str(golden("treefit_edges.npz")["sklearn_version"])
    if sklearn.__version__ != want:
        pytest.skip("the builder restates scikit-learn %s; %s is installed" % (want, sklearn.__version__))
    return sklearn


def golden_case(g, i):
    p = "c%d_" % i
    return {k: g[p + k] for k in ("X", "y", "w", "mean", "scale")} | {"seed": int(g[p + "seed"])}


def same_tree(got, g, prefix, what):
    for f in FIELDS:
        a, b = np.asarray(got[f]), g[prefix + f]
        assert a.shape == b.shape, (what, f, a.shape, b.shape)
        if b.dtype.kind == "f":
            assert a.dtype == np.float64 and np.array_equal(a.view(np.int64), b.view(np.int64)), (what, f)      # bit for bit
        else:
            assert np.array_equal(a, b), (what, f)


def test_cases_in_the_tree_are_the_recorded_ones():
    g = golden("treefit_edges.npz")
    cases = R.edge_cases()
    assert str(g["kind"]) == "treefit" and list(g["names"]) == list(cases)
    for i, (name, case) in enumerate(cases.items()):
        for k, v in golden_case(g, i).items():
            assert np.array_equal(v, case[k]), (name, k)
    lim = R.limit_case()
    g = golden("treefit_limit.npz")
    assert np.array_equal(g["c0_X"].astype(np.float64), lim["X"]) and np.array_equal(g["c0_y"], lim["y"]) and int(g["c0_seed"]) == lim["seed"]
    assert lim["X"].shape[0] == aT.TREE_MAX_ROWS


@pytest.mark.parametrize("splitter", ["best", "random"])
def test_restatement_equals_the_goldens(splitter):
    g = golden("treefit_edges.npz")
    for i, name in enumerate(g["names"]):
        c = golden_case(g, i)
        k = int(np.unique(c["y"]).shape[0])
        got = R.fit_tree(R.standardize32(c["X"], c["mean"], c["scale"]), c["y"], c["w"], k, c["seed"], splitter)
        same_tree(got, g, "c%d_%s_" % (i, splitter), name)
    # what the cases are there for
    names = list(g["names"])
    at = lambda name, f: g["c%d_%s_%s" % (names.index(name), splitter, f)]        # noqa: E731
    assert at("one_in_bag_row", "feature").shape == (1,) and at("one_in_bag_row", "value").shape == (1, 2)
    assert at("one_class", "value").tolist() == [[1.0]]
    assert at("two_rows", "feature").tolist() == [0, -2, -2]
    assert at("all_constant", "feature").tolist() == [-2] and at("all_constant", "impurity")[0] > 0.6      # an impure leaf
    assert set(at("three_of_five_constant", "feature").tolist()) <= {-2, 1, 3}
    depth_bound = at("chain_300", "feature").shape[0]
    assert depth_bound == 599                                                       # 300 leaves: every row its own
    assert at("classes_64", "value").shape[1] == 64
    if splitter == "random":                                                        # the root's draw returned RAND_R_MAX: threshold = min
        assert at("threshold_equals_max", "threshold")[0] == 0.0 and at("threshold_equals_max", "n_node_samples")[1] == 1


@pytest.mark.parametrize("splitter", ["best", "random"])
def test_restatement_equals_live_scikit_learn(splitter):
    live_sklearn()
    for name, c in R.edge_cases().items():
        k = int(np.unique(c["y"]).shape[0])
        x32 = R.standardize32(c["X"], c["mean"], c["scale"])
        ref, seed = R.sklearn_tree(x32, c["y"], c["w"], k, R.FixedSeed(c["seed"]), splitter)
        got = R.fit_tree(x32, c["y"], c["w"], k, seed, splitter)
        for f in FIELDS:
            assert np.asarray(got[f]).shape == ref[f].shape and np.array_equal(got[f], ref[f]), (name, f)
    rng = np.random.default_rng(8)                                                  # and through an integer random_state
    X, y, w = rng.standard_normal((150, 9)), rng.integers(0, 3, 150), R.bootstrap_weights(11, 150)
    y[:3] = [0, 1, 2]
    w[:3] = np.maximum(w[:3], 1)
    ref, seed = R.sklearn_tree(X.astype(np.float32), y, w, 3, 11, splitter)
    assert seed == aT.tree_inputs(11, 150, False)[0]
    got = R.fit_tree(X.astype(np.float32), y, w, 3, seed, splitter)
    for f in FIELDS:
        assert np.array_equal(got[f], ref[f]), f


def test_declared_feature_threshold_has_no_effect_in_scikit_learn():
    """_partitioner.pxd declares FEATURE_THRESHOLD = 1e-7; the compiled scikit-learn compares against 0.  The kernel and the
    restatement follow the library, not the declaration: two adjacent float32 values are split."""
    live_sklearn()
    from sklearn.tree import DecisionTreeClassifier, ExtraTreeClassifier
    a = np.float32(0.1)
    X = np.array([[a], [a], [np.nextafter(a, np.float32(1))], [np.nextafter(a, np.float32(1))]], dtype=np.float32)
    for cls in (DecisionTreeClassifier, ExtraTreeClassifier):
        assert cls(random_state=0).fit(X, [0, 0, 1, 1]).tree_.node_count == 3


def test_host_seed_and_bootstrap_derivation_equals_scikit_learns():
    g = golden("treefit_sweep.npz")
    seed, ne, n = int(g["j2_seed"]), int(g["j2_n_estimators"]), g["j2_train"].shape[0]
    states = aT.forest_tree_seeds(seed, ne)
    assert states == g["j2_tree_states"].tolist()
    for t, s in enumerate(states):
        rand_r, w = aT.tree_inputs(s, n, True)
        assert np.array_equal(w, g["j2_in_bag"][t]) and w.dtype == np.int32 and w.sum() == n
        assert rand_r == R.splitter_seed(s) and aT.tree_inputs(s, n, False) == (rand_r, None)
    assert aT.forest_tree_seeds(np.random.RandomState(seed), ne) == states
    np.random.seed(seed)                                                            # None: NumPy's global state, as check_random_state(None)
    assert aT.forest_tree_seeds(None, ne) == states
    sklearn_ensemble = live_sklearn() and pytest.importorskip("sklearn.ensemble")
    X, y, jobs = R.sweep_case()
    tr = jobs[2][0]
    m = sklearn_ensemble.RandomForestClassifier(n_estimators=ne, random_state=seed).fit(X[tr], y[tr])
    assert [e.random_state for e in m.estimators_] == states
    for e, s in zip(m.estimators_samples_, states):
        assert np.array_equal(np.bincount(e, minlength=n), aT.tree_inputs(s, n, True)[1])


def test_sweep_golden_is_the_case_in_the_tree():
    g = golden("treefit_sweep.npz")
    X, y, jobs = R.sweep_case()
    assert np.array_equal(g["X"], X) and np.array_equal(g["y"], y) and int(g["n_jobs"]) == len(jobs) == 7
    for j, job in enumerate(jobs):
        for name, v in zip(("train", "test", "mean", "scale"), job[:4]):
            assert np.array_equal(g["j%d_%s" % (j, name)], v)
        assert (int(g["j%d_n_estimators" % j]), int(g["j%d_seed" % j])) == job[4]
    assert 2.0 not in y[jobs[6][0]] and g["j6_randomforest_proba"].shape == (30, 2)     # a training list that lacks a class


@pytest.mark.parametrize("kind", ["randomforest", "extratrees"])
def test_to_sklearn_forest_predicts_and_pickles_like_the_model(kind):
    sklearn_ensemble = pytest.importorskip("sklearn.ensemble")
    X, y, jobs = R.sweep_case()
    cls = sklearn_ensemble.RandomForestClassifier if kind == "randomforest" else sklearn_ensemble.ExtraTreesClassifier
    m = cls(n_estimators=7, random_state=5).fit(X[:300], y[:300])
    arrays = aT.forest_arrays(m)
    arrays.impurity = np.concatenate([e.tree_.impurity for e in m.estimators_])
    arrays.n_node_samples = np.concatenate([e.tree_.n_node_samples for e in m.estimators_])
    arrays.weighted_n_node_samples = np.concatenate([e.tree_.weighted_n_node_samples for e in m.estimators_])
    back = aT.to_sklearn_forest(arrays, kind)
    assert type(back) is cls and len(back.estimators_) == 7
    assert np.array_equal(back.predict(X[300:]), m.predict(X[300:])) and np.array_equal(back.predict_proba(X[300:]), m.predict_proba(X[300:]))
    for a, b in zip(back.estimators_, m.estimators_):
        assert a.tree_.max_depth == b.tree_.max_depth and a.tree_.node_count == b.tree_.node_count
        for f in FIELDS:
            assert np.array_equal(getattr(a.tree_, f), getattr(b.tree_, f)), f
    again = pickle.loads(pickle.dumps(back))                                        # the reference's model format: a pickled classifier
    assert np.array_equal(again.predict_proba(X[300:]), m.predict_proba(X[300:]))
    assert aT.is_forest(again) and np.array_equal(aT.forest_arrays(again).threshold, arrays.threshold)
    bare = aT.to_sklearn_forest(aT.forest_arrays(m), kind)                          # without the training statistics: zeros, same predictions
    assert np.array_equal(bare.predict_proba(X[300:]), m.predict_proba(X[300:]))
    with pytest.raises(ValueError):
        aT.to_sklearn_forest(arrays, "gradientboosting")


def test_python_keywords_are_refused_before_any_work():
    feats = train_ref.three_class_features()
    for kind in ("knn", "svm", "svm_rbf", "gradientboosting"):
        with pytest.raises(ValueError, match="forest_fit"):
            aT.evaluate_classifier(feats, ["a", "b", "c"], kind, [1], 0, forest_fit="device")
        with pytest.raises(ValueError, match="forest_fit"):
            aT.extract_features_and_train(["x"], 1.0, 1.0, 0.05, 0.05, kind, "model", forest_fit="device")
    for kind in ("randomforest", "extratrees"):
        with pytest.raises(ValueError, match="forest_fit"):
            aT.evaluate_classifier(feats, ["a", "b", "c"], kind, [1], 0, forest_fit="gpu")
        with pytest.raises(ValueError, match="forest_fit"):
            aT.extract_features_and_train(["x"], 1.0, 1.0, 0.05, 0.05, kind, "model", forest_fit="gpu")
        with pytest.raises(ValueError):                   # the SVM keywords keep refusing the forests
            aT.evaluate_classifier(feats, ["a", "b", "c"], kind, [1], 0, svm_fit="device")
        with pytest.raises(NotImplementedError):          # and SMOTE stays refused
            aT.evaluate_classifier(feats, ["a", "b", "c"], kind, [1], 0, smote=True, forest_fit="device")
    with pytest.raises(TypeError):                        # keyword only
        aT.evaluate_classifier(feats, ["a", "b", "c"], "randomforest", [1], 0, None, -1, 0.9, False, "sklearn", "device")


def test_python_entry_points_reject_bad_arguments_without_a_device():
    X = np.zeros((6, 3))
    y = np.array([0., 1, 0, 1, 0, 1])
    job = (np.array([0, 1, 2]), np.array([3, 4]), np.zeros(3), np.ones(3), (3, 1))
    for args in ((np.zeros(6), y, [job]), (X, y[:5], [job]), (X, y, []), (X, y, [job[:4]]), (X, y, [(job[0], job[1], np.zeros(2), np.ones(3), (3, 1))])):
        with pytest.raises(ValueError):
            aT.forest_split_fit_predict(*args, "randomforest")
    with pytest.raises(ValueError):
        aT.forest_split_fit_predict(X, y, [job], "gradientboosting")
    with pytest.raises(ValueError):                       # the library's argument errors
        aT.forest_split_fit_predict(X, y, [(job[0], job[1], job[2], job[3], (0, 1))], "extratrees")
    with pytest.raises(ValueError):
        aT.forest_split_fit_predict(X, y, [(np.array([0, 9]), job[1], job[2], job[3], (3, 1))], "extratrees")
    task = (np.array([0, 1, 2]), np.array([0, 1, 0]), None, 7, np.zeros(3), np.ones(3))
    for tasks in ([], [task[:5]], [(task[0], task[1][:2]) + task[2:]], [task[:2] + (np.array([1.0, 1.0, 1.0]),) + task[3:]],
                  [task[:2] + (np.array([0, 0, 0]),) + task[3:]], [task[:2] + (np.array([1, -1, 1]),) + task[3:]],
                  [task[:2] + (np.array([1, aT.TREE_MAX_WEIGHT + 1, 1]),) + task[3:]], [task[:3] + (-1,) + task[4:]], [task[:3] + (2**32,) + task[4:]]):
        with pytest.raises(ValueError):
            aT.tree_fit(X, tasks, "best")
    with pytest.raises(ValueError):
        aT.tree_fit(X, [task], "gini")
    # the row limit: refused in Python, before the library is asked
    n = aT.TREE_MAX_ROWS + 1
    big, labels = np.zeros((n, 2)), np.arange(n) % 2
    with pytest.raises(NotImplementedError, match="8192"):
        aT.tree_fit(big, [(np.arange(n), labels, None, 1, np.zeros(2), np.ones(2))], "random")
    with pytest.raises(NotImplementedError, match="8192"):
        aT.train_forest_device(big, labels, 3, "extratrees", random_state=0)
    with pytest.raises(NotImplementedError, match="8192"):
        aT.forest_split_fit_predict(big, labels, [(np.arange(n), np.arange(2), np.zeros(2), np.ones(2), (1, 0))], "randomforest")
    for args in ((np.zeros(6), y, 3), (X, y[:5], 3), (X, y, 0)):
        with pytest.raises(ValueError):
            aT.train_forest_device(*args)
    with pytest.raises(ValueError):
        aT.train_forest_device(X, y, 3, "gradientboosting")


def _p(a, kind):
    return None if a is None else a.ctypes.data_as(kind)


def _i32(*v):
    return np.array(v, dtype=np.int32)


def _i64(*v):
    return np.array(v, dtype=np.int64)


class _Tasks:
    """A valid call of paa_tree_fit_tasks_f64 (two jobs, three trees) whose arguments can be replaced one at a time."""

    def __init__(self):
        self.n_samples, self.n_dims, self.n_jobs, self.n_tasks, self.splitter = 6, 3, 2, 3, 0
        self.X = np.zeros((6, 3))
        self.job_off, self.job_idx, self.job_label, self.job_k = _i64(0, 3, 5), _i32(0, 1, 2, 3, 4), _i32(0, 1, 0, 1, 0), _i32(2, 2)
        self.mean, self.std = np.zeros((2, 3)), np.ones((2, 3))
        self.task_job, self.task_seed, self.task_weight = _i32(0, 1, 0), _i64(1, 2, 3), _i32(1, 1, 1, 2, 0, 0, 1, 1)
        self.total_nodes, self.total_values = 5 + 1 + 3, 2 * (5 + 1 + 3)
        self.job_flags, self.node_count = np.zeros(2, dtype=np.int32), np.zeros(3, dtype=np.int32)
        for name in ("children_left", "children_right", "feature", "n_node_samples"):
            setattr(self, name, np.zeros(9, dtype=np.int32))
        for name in ("threshold", "impurity", "weighted"):
            setattr(self, name, np.zeros(9))
        self.missing, self.value = np.zeros(9, dtype=np.uint8), np.zeros(18)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        return _ffi.lib().paa_tree_fit_tasks_f64(
            _p(self.X, _ffi.c_f64p), self.n_samples, self.n_dims, self.n_jobs, _p(self.job_off, _ffi.c_i64p), _p(self.job_idx, _ffi.c_i32p),
            _p(self.job_label, _ffi.c_i32p), _p(self.job_k, _ffi.c_i32p), _p(self.mean, _ffi.c_f64p), _p(self.std, _ffi.c_f64p), self.n_tasks,
            _p(self.task_job, _ffi.c_i32p), _p(self.task_seed, _ffi.c_i64p), _p(self.task_weight, _ffi.c_i32p), self.splitter, self.total_nodes,
            self.total_values, _p(self.job_flags, _ffi.c_i32p), _p(self.node_count, _ffi.c_i32p), _p(self.children_left, _ffi.c_i32p),
            _p(self.children_right, _ffi.c_i32p), _p(self.feature, _ffi.c_i32p), _p(self.threshold, _ffi.c_f64p), _p(self.impurity, _ffi.c_f64p),
            _p(self.n_node_samples, _ffi.c_i32p), _p(self.weighted, _ffi.c_f64p), _p(self.missing, C.POINTER(C.c_uint8)), _p(self.value, _ffi.c_f64p))


class _Splits:
    """A valid two-job call of paa_forest_fit_splits_f64 whose arguments can be replaced one at a time."""

    def __init__(self):
        self.n_samples, self.n_dims, self.n_jobs, self.splitter, self.max_classes = 6, 3, 2, 0, 3
        self.X = np.zeros((6, 3))
        self.labels = _i32(0, 1, 0, 1, 2, 1)
        self.train_off, self.train_idx = _i64(0, 3, 6), _i32(0, 1, 2, 3, 4, 5)
        self.test_off, self.test_idx = _i64(0, 2, 3), _i32(4, 5, 0)
        self.mean, self.std = np.zeros((2, 3)), np.ones((2, 3))
        self.n_estimators, self.tree_seed, self.tree_weight = _i32(2, 1), _i64(1, 2, 3), _i32(1, 1, 1, 0, 2, 1, 3, 0, 0)
        self.label_out, self.proba, self.job_flags = np.zeros(3, dtype=np.int32), np.zeros((3, 3)), np.zeros(2, dtype=np.int32)

    def __call__(self, **replace):
        for k, v in replace.items():
            assert hasattr(self, k)
            setattr(self, k, v)
        return _ffi.lib().paa_forest_fit_splits_f64(
            _p(self.X, _ffi.c_f64p), self.n_samples, self.n_dims, _p(self.labels, _ffi.c_i32p), self.n_jobs, _p(self.train_off, _ffi.c_i64p),
            _p(self.train_idx, _ffi.c_i32p), _p(self.test_off, _ffi.c_i64p), _p(self.test_idx, _ffi.c_i32p), _p(self.mean, _ffi.c_f64p),
            _p(self.std, _ffi.c_f64p), _p(self.n_estimators, _ffi.c_i32p), self.splitter, _p(self.tree_seed, _ffi.c_i64p),
            _p(self.tree_weight, _ffi.c_i32p), _p(self.label_out, _ffi.c_i32p), _p(self.proba, _ffi.c_f64p), self.max_classes,
            _p(self.job_flags, _ffi.c_i32p), None)


needs_no_device = pytest.mark.skipif(_ffi.device_count() > 0, reason="a GPU is present: the valid call would run")


def test_c_abi_rejects_bad_tree_tasks_before_any_device_work():
    names = ("X", "job_off", "job_idx", "job_label", "job_k", "mean", "std", "task_job", "task_seed", "task_weight", "job_flags", "node_count",
             "children_left", "children_right", "feature", "threshold", "impurity", "n_node_samples", "weighted", "missing", "value")
    for name in names:
        assert _Tasks()(**{name: None}) == _ffi.ERR_ARG, name
    bad = [dict(job_off=_i64(1, 3, 5)), dict(job_off=_i64(0, 3, 2)), dict(job_off=_i64(0, 0, 5)), dict(job_idx=_i32(0, 1, 2, 3, 6)),
           dict(job_idx=_i32(0, -1, 2, 3, 4)), dict(job_label=_i32(0, 2, 0, 1, 0)), dict(job_label=_i32(0, -1, 0, 1, 0)), dict(job_k=_i32(2, 0)),
           dict(n_dims=0), dict(splitter=2), dict(splitter=-1), dict(n_tasks=0), dict(n_jobs=0), dict(n_samples=0), dict(n_samples=2**31),
           dict(task_job=_i32(0, 2, 0)), dict(task_job=_i32(0, -1, 0)), dict(task_seed=_i64(1, -1, 3)), dict(task_seed=_i64(1, 2**32, 3)),
           dict(task_weight=_i32(1, 1, 1, 0, 0, 0, 1, 1)),                       # tree 1: nothing in the bag
           dict(task_weight=_i32(1, -1, 1, 2, 0, 0, 1, 1)), dict(task_weight=_i32(1, 8192, 1, 2, 0, 0, 1, 1)),
           dict(total_nodes=10), dict(total_values=17)]
    for kw in bad:
        assert _Tasks()(**kw) == _ffi.ERR_ARG, kw
        assert _ffi.last_error()
    # beyond the limits: refused with the limit in the message, no other path
    assert _Tasks()(n_dims=257) == _ffi.ERR_UNSUPPORTED and "256" in _ffi.last_error()
    assert _Tasks()(job_k=_i32(65, 2)) == _ffi.ERR_UNSUPPORTED and "64" in _ffi.last_error()
    geo = aT.tree_fit_geometry()
    assert geo == (256, aT.TREE_MAX_ROWS, 64, 256, aT.TREE_MAX_WEIGHT, 1024)
    n = geo[1] + 1
    assert _Tasks()(n_jobs=1, n_tasks=1, job_off=_i64(0, n), job_idx=np.zeros(n, dtype=np.int32), job_label=np.zeros(n, dtype=np.int32),
                    task_weight=np.ones(n, dtype=np.int32)) == _ffi.ERR_UNSUPPORTED
    assert "8192" in _ffi.last_error()
    assert _ffi.lib().paa_debug_tree_fit_geometry(None) == _ffi.ERR_ARG
    header = open(os.path.join(ROOT, "include", "paa_hip.h")).read()
    assert "#define PAA_TREE_MAX_ROWS 8192" in header and "#define PAA_TREE_MAX_WEIGHT 8191" in header


def test_c_abi_rejects_bad_forest_split_jobs_before_any_device_work():
    for name in ("X", "labels", "train_off", "train_idx", "test_off", "test_idx", "mean", "std", "n_estimators", "tree_seed", "label_out", "job_flags"):
        assert _Splits()(**{name: None}) == _ffi.ERR_ARG, name
    bad = [dict(train_off=_i64(1, 3, 6)), dict(test_off=_i64(-1, 2, 3)), dict(train_off=_i64(0, 4, 3)), dict(test_off=_i64(0, 2, 1)),
           dict(train_idx=_i32(0, 1, 2, 3, 4, 6)), dict(train_idx=_i32(0, -1, 2, 3, 4, 5)), dict(test_idx=_i32(4, 6, 0)), dict(n_dims=0),
           dict(splitter=3), dict(n_jobs=0), dict(n_samples=0), dict(labels=_i32(0, -1, 0, 1, 2, 1)), dict(train_off=_i64(0, 0, 6)),
           dict(n_estimators=_i32(2, 0)), dict(tree_seed=_i64(1, 2, -3)), dict(tree_weight=_i32(1, 1, 1, 0, 0, 0, 3, 0, 0)),
           dict(tree_weight=_i32(1, 1, 1, 0, 2, 1, 8192, 0, 0)), dict(max_classes=1), dict(test_off=_i64(0, 2, 2**31))]
    for kw in bad:
        assert _Splits()(**kw) == _ffi.ERR_ARG, kw
        assert _ffi.last_error()
    assert _Splits()(n_dims=257) == _ffi.ERR_UNSUPPORTED and "256" in _ffi.last_error()


@needs_no_device
def test_valid_calls_reach_the_device_and_fail_there():
    """The templates above are valid: without a device they pass every check and stop at the missing device."""
    assert _Tasks()() == _ffi.ERR_HIP and _Splits()() == _ffi.ERR_HIP and _Splits()(tree_weight=None, proba=None) == _ffi.ERR_HIP


def test_new_symbols_are_declared_and_built():
    from pyaudioanalysis_amd import _build
    header = open(os.path.join(ROOT, "include", "paa_hip.h")).read()
    for s in ("paa_tree_fit_tasks_f64", "paa_forest_fit_splits_f64", "paa_debug_tree_fit_geometry"):
        assert s in _ffi.EXPORTED_SYMBOLS and hasattr(_ffi.lib(), s) and ("int %s(" % s) in header, s
    assert "kernels_treefit.hpp" in _build.HEADERS and "lib_treefit.hpp" in _build.HEADERS
    unit = open(os.path.join(ROOT, "pyaudioanalysis_amd", "csrc", "family_forest.hip")).read()
    assert '#include "kernels_treefit.hpp"' in unit                                 # compiled in the forest unit: no new .hip file
