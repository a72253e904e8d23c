"""GPU checks of the tree builder (tree_fit_kernel, kernels_treefit.hpp) and of the forest sweeps (forest_fit_splits,
lib_treefit.hpp) where the small cases of test_treefit_gpu.py / test_treefit_reg_gpu.py do not reach:
 A  the classifier's largest launch -- 8192 rows, 64 classes, 128 histogram columns, ~132 KB of dynamic LDS, weights up to the
    limit 8191 -- against scikit-learn's own trees (tests/golden/treefit_wide.npz), integers equal and floats bit-equal.  The same
    rows with 32 classes (the full 32 x 257 histogram) are NOT a golden: with them the file would pass the largest golden in the
    tree, so that tree is walked on the host (treefit_ref.check_gini_tree) and held to test C;
 B  255 and 256 dims and the weights 0 / 1 / 2 / 8191 against the restatement treefit_ref.fit_tree;
 C  one tree, byte for byte, across every launch shape: alone, beside a 5-row filler, beside the 8192-row 64-class filler
    (hist_cols 128, lds_keys 8192), beside a 33-class and a 32-class filler (the two sides of the column switch); the regressor
    beside its 8192-row golden;
 D  sweeps that need three chunks of the real 1 GiB scratch bound (the count is derived by treefit_ref.expected_chunks from the
    rule, not read from the library), against (a) every job submitted alone, (b) the trees rebuilt by tree_fit and scored in NumPy,
    (c) live scikit-learn where it is installed in the recorded version;
 E  a job with more test rows than one traversal pass (32 768)."""
import functools

import numpy as np
import pytest

import treefit_ref as R
import treefit_reg_ref as RR
from pyaudioanalysis_amd import audioTrainTest as aT
from test_treefit_cpu import FIELDS, golden, golden_case, same_tree
from test_treefit_gpu import fit_cases, task_of
from test_treefit_reg_cpu import same_tree as same_reg_tree
from test_treefit_reg_gpu import fit_cases as fit_reg_cases, general_cases

pytestmark = pytest.mark.gpu


def same_bytes(got, want, what):
    for f in FIELDS:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, f)


def widened(c, d):
    """The case with constant columns appended up to d dims."""
    more = d - c["X"].shape[1]
    return dict(c, X=np.pad(np.asarray(c["X"], dtype=np.float64), ((0, 0), (0, more))), mean=np.pad(c["mean"], (0, more)),
                scale=np.pad(c["scale"], (0, more), constant_values=1.0))


def sklearn_as_recorded(g):
    try:
        import sklearn
    except ImportError:
        return False
    return sklearn.__version__ == str(g["sklearn_version"])


# ---- A: the largest launch

@pytest.mark.parametrize("splitter", ["best", "random"])
def test_the_row_limit_with_64_classes_equals_scikit_learns_tree(gpu_lib, splitter):
    g = golden("treefit_wide.npz")
    c = golden_case(g, 0)
    assert c["X"].shape == (aT.tree_fit_geometry()[1], 3) and np.unique(c["y"]).shape[0] == aT.tree_fit_geometry()[2] and c["w"].max() == aT.tree_fit_geometry()[4]
    res = aT.tree_fit(c["X"].astype(np.float64), [task_of(c)], splitter)
    assert res.classes[0].tolist() == list(range(64))
    same_tree(res.trees[0], g, "c0_%s_" % splitter, "wide limit")


@functools.lru_cache(maxsize=None)
def wide32_alone(splitter):
    c = R.wide_limit_case(32)
    return aT.tree_fit(c["X"], [task_of(c)], splitter).trees[0]


@pytest.mark.parametrize("splitter", ["best", "random"])
def test_the_row_limit_with_32_classes_passes_the_host_walk(gpu_lib, splitter):
    """The 256-column histogram at its largest, k_max > 32 from below: counts, values, impurities and leaves of every node."""
    c = R.wide_limit_case(32)
    tree = wide32_alone(splitter)
    assert tree["value"].shape[1] == 32
    leaves = R.check_gini_tree(tree, R.standardize32(c["X"], c["mean"], c["scale"]), c["y"], c["w"], 32)
    assert leaves == (tree["feature"].shape[0] + 1) // 2 and leaves > 2000


# ---- B: dims and weights

@pytest.mark.parametrize("splitter", ["best", "random"])
def test_255_and_256_dims_and_the_weight_limit_equal_the_restatement(gpu_lib, splitter):
    cases = R.dims_and_weight_cases()
    assert max(c["X"].shape[1] for c in cases.values()) == aT.tree_fit_geometry()[3] and max(c["w"].max() for c in cases.values()) == aT.tree_fit_geometry()[4]
    for (name, c), tree in zip(cases.items(), fit_cases(list(cases.values()), splitter)):
        ref = R.fit_tree(R.standardize32(c["X"], c["mean"], c["scale"]), c["y"], c["w"], 3, c["seed"], splitter)
        for f in FIELDS:
            a, b = np.asarray(tree[f]), np.asarray(ref[f])
            assert a.shape == b.shape and np.array_equal(a, b), (name, f)
            assert b.dtype.kind != "f" or a.tobytes() == b.astype(np.float64).tobytes(), (name, f)


# ---- C: one tree, every launch shape

def class_filler(n, k, d, seed):
    rs = np.random.RandomState(seed)
    y = np.arange(n) % k
    return dict(X=np.round(rs.randn(n, d) * 16) / 16 + 0.25 * (y % 5)[:, None], y=y, w=np.ones(n, dtype=np.int32), mean=np.zeros(d),
                scale=np.ones(d), seed=seed)


@pytest.mark.parametrize("splitter", ["best", "random"])
def test_a_classifier_tree_has_the_same_bits_in_every_launch_shape(gpu_lib, splitter):
    g = golden("treefit_edges.npz")
    names = [str(s) for s in g["names"]]
    at = names.index("weights_0_1_2")
    target = golden_case(g, at)
    d = target["X"].shape[1]
    wide = widened(R.wide_limit_case(), d)
    alone = fit_cases([target], splitter)[0]
    same_tree(alone, g, "c%d_%s_" % (at, splitter), "alone")
    launches = (("5 rows, 2 classes", [class_filler(5, 2, d, 1), target], 1),
                ("8192 rows, 64 classes, target last", [wide, target], 1),
                ("8192 rows, 64 classes, target first", [target, wide], 0),
                ("33 classes", [class_filler(200, 33, d, 2), target], 1),
                ("32 classes", [target, class_filler(200, 32, d, 3)], 0))
    for what, cases, place in launches:
        same_bytes(fit_cases(cases, splitter)[place], alone, what)
    # and the 32-class tree of the largest 256-column launch beside a 64-class filler, which moves it to 128 columns
    c32 = R.wide_limit_case(32)
    same_bytes(fit_cases([class_filler(200, 64, 3, 4), c32], splitter)[1], wide32_alone(splitter), "32 classes at the row limit")


def test_a_regression_tree_has_the_same_bits_in_every_launch_shape(gpu_lib):
    """The target's sums ROUND, so the order of every sum shows."""
    target = dict(general_cases()[2])
    d = target["X"].shape[1]
    g = golden("treefit_reg_limit.npz")
    limit = golden_case(g, 0)
    limit["X"] = limit["X"].astype(np.float64)
    wide = widened(R.wide_limit_case(), d)
    wide["y"] = wide["y"].astype(np.float64)
    tiny = dict(X=np.arange(5.0 * d).reshape(5, d) % 7, y=np.array([0.5, -1.25, 3.0, 3.0, 0.1]), w=np.ones(5, dtype=np.int32), mean=np.zeros(d),
                scale=np.ones(d), seed=5)
    assert limit["X"].shape == (aT.tree_fit_geometry()[1], d)
    alone = fit_reg_cases([target])[0]
    for what, cases, place in (("5 rows", [tiny, target], 1), ("the classifier's 8192 rows", [wide, target], 1),
                               ("the 8192-row golden, target last", [limit, target], 1), ("the 8192-row golden, target first", [target, limit], 0)):
        trees = fit_reg_cases(cases)
        same_bytes(trees[place], alone, what)
        if cases[1 - place] is limit:                                               # the filler is still scikit-learn's tree
            same_reg_tree(trees[1 - place], g, "c0_", "row limit beside a small task")


# ---- D: the sweep across chunks

def rebuilt(X, y, job, kind, rows):
    """Reference (b): the job's trees by tree_fit / tree_fit_regression from the seeds and weights the sweep derives, scored in NumPy
    on the float32 rows X[rows] standardised with the job's statistics."""
    tasks = R.job_tasks(y, job, kind != "extratrees", aT.forest_tree_seeds, aT.tree_inputs)
    fit = aT.tree_fit_regression(X, tasks) if kind == "regressor" else aT.tree_fit(X, tasks, kind)
    assert len(fit.trees) == job[4][0]
    return fit, R.score_trees(fit.trees, R.standardize32(X[rows], job[2], job[3]))


@pytest.mark.parametrize("kind", ["randomforest", "extratrees"])
def test_classifier_sweep_across_three_chunks(gpu_lib, kind):
    X, y, jobs = R.chunk_sweep_case(kind)
    chunks = R.expected_chunks(jobs, kind, y)
    assert len(chunks) >= 3 and chunks == R.CHUNK_LAYOUT                            # a condition of the test, from the rule
    res = aT.forest_split_fit_predict(X, y, jobs, kind, proba=True)
    assert res.n_chunks == len(chunks) and res.proba.shape == (sum(len(j[1]) for j in jobs), 64)
    tiny = R.CHUNK_TINY
    assert res.classes[tiny].tolist() == [17, 40] and set(res.job(tiny)[0].tolist()) <= {17, 40} and res.job(tiny)[1].shape == (7, 2)
    assert np.all(res.proba[res._rows(tiny), 2:] == 0.0) and np.all(res.job(tiny)[1].sum(1) == 1.0)
    assert res.job(R.CHUNK_NO_TEST)[0].shape == (0,)
    for j, job in enumerate(jobs):                                                  # (a) every job alone: one chunk, the path the goldens hold
        alone = aT.forest_split_fit_predict(X, y, [job], kind, proba=True)
        assert alone.n_chunks == 1
        (label, proba), (label1, proba1) = res.job(j), alone.job(0)
        assert np.array_equal(label, label1), j
        assert proba.shape == proba1.shape and proba.tobytes() == proba1.tobytes(), j
    for j in (2, tiny, 6):                                                          # (b) the trees rebuilt, scored in NumPy
        fit, P = rebuilt(X, y, jobs[j], kind, jobs[j][1])
        label, proba = res.job(j)
        assert np.array_equal(label, fit.classes[0][np.argmax(P, axis=1)]), j
        assert proba.shape == P.shape and proba.tobytes() == P.tobytes(), j
    if sklearn_as_recorded(golden("treefit_wide.npz")):                           # (c)
        for j in (tiny, 4):
            label, proba, _ = R.sklearn_forest(X, y, jobs[j], kind)
            assert np.array_equal(res.job(j)[0], label) and np.array_equal(res.job(j)[1], proba), j


def test_regressor_sweep_across_three_chunks(gpu_lib):
    X, y, jobs = RR.chunk_sweep_case()
    chunks = R.expected_chunks(jobs, "regressor")
    assert len(chunks) >= 3 and chunks == RR.CHUNK_LAYOUT
    res = aT.forest_regression_split_fit_predict(X, y, jobs, train_pred=True)
    assert res.n_chunks == len(chunks) and res.pred.shape == (sum(len(j[1]) for j in jobs),) and res.train_pred.shape == (sum(len(j[0]) for j in jobs),)
    for j, job in enumerate(jobs):                                                  # (a)
        alone = aT.forest_regression_split_fit_predict(X, y, [job], train_pred=True)
        assert alone.n_chunks == 1
        for got, want in zip(res.job(j), alone.job(0)):
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), j
    for j in (1, RR.CHUNK_TINY, 4, 6):                                              # (b) a job of every chunk, none the first of its chunk
        rows = np.concatenate([jobs[j][1], jobs[j][0]])
        _, P = rebuilt(X, y, jobs[j], "regressor", rows)
        pred, train_pred = res.job(j)
        assert np.concatenate([pred, train_pred]).tobytes() == P[:, 0].tobytes(), j
    if sklearn_as_recorded(golden("treefit_reg_sweep.npz")):                      # (c) exact targets: scikit-learn's bits
        pred, train_pred, _ = RR.sklearn_forest(X, y, jobs[RR.CHUNK_TINY])
        assert np.array_equal(res.job(RR.CHUNK_TINY)[0], pred) and np.array_equal(res.job(RR.CHUNK_TINY)[1], train_pred)


# ---- E: more test rows than one traversal pass

def test_more_test_rows_than_one_traversal_pass(gpu_lib):
    X, labels, y, job = RR.many_test_rows_case()
    edge = slice(32767, 32774)
    res = aT.forest_split_fit_predict(X, labels, [job], "extratrees", proba=True)
    fit, P = rebuilt(X, labels, job, "extratrees", job[1])
    assert res.n_chunks == 1 and res.proba.shape == (32774, 3) == P.shape
    assert np.array_equal(res.label[edge], fit.classes[0][np.argmax(P[edge], axis=1)]) and res.proba[edge].tobytes() == P[edge].tobytes()
    assert np.array_equal(res.label, fit.classes[0][np.argmax(P, axis=1)]) and res.proba.tobytes() == P.tobytes()
    assert np.unique(res.label).shape[0] == 3
    reg = aT.forest_regression_split_fit_predict(X, y, [job], train_pred=True)
    _, P = rebuilt(X, y, job, "regressor", np.concatenate([job[1], job[0]]))
    assert reg.pred.shape == (32774,) and reg.train_pred.shape == (60,)
    assert reg.pred[edge].tobytes() == P[edge, 0].tobytes()
    assert reg.pred.tobytes() == P[:32774, 0].tobytes() and reg.train_pred.tobytes() == P[32774:, 0].tobytes()
    assert np.unique(reg.pred).shape[0] > 10
