"""GPU checks of the regression-tree builder (the squared-error instance of tree_fit_kernel through paa_tree_fit_reg_tasks_f64 /
audioTrainTest.tree_fit_regression), of the regression sweep built on it (paa_forest_reg_fit_splits_f64 /
forest_regression_split_fit_predict, evaluate_regression(forest_fit="device")) and of the final fit
(train_random_forest_regression_device, to_sklearn_forest_regressor, feature_extraction_train_regression(forest_fit="device")).
Two acceptances, as the kernel's contract has two halves.  Targets that make every sum of the criterion exact in FP64 (all goldens:
multiples of 1/8 within +-1024, total weight <= 8192): EQUALITY with scikit-learn 1.7.2's own trees, integer arrays equal, float64
arrays bit-equal.  General targets: every tree is walked on the host with exact arithmetic and held to what CART demands, with
derived bounds (treefit_reg_ref.check_cart_tree); and the same task gives the same bits alone and anywhere in a batch."""
import os

import numpy as np
import pytest

import treefit_reg_ref as R
from pyaudioanalysis_amd import audioTrainTest as aT
from test_treefit_cpu import golden, golden_case
from test_treefit_reg_cpu import FIELDS, live_sklearn, same_tree
from test_treefit_gpu import _after
from test_train_gpu import _run

pytestmark = pytest.mark.gpu


def task_of(c):
    return (np.arange(c["X"].shape[0]), c["y"], c["w"], c["seed"], c["mean"], c["scale"])


def fit_cases(cases):
    """Every case a task of ONE call: the cases stacked into one sample matrix per width."""
    out = [None] * len(cases)
    for d in sorted({c["X"].shape[1] for c in cases}):
        group = [i for i, c in enumerate(cases) if c["X"].shape[1] == d]
        X = np.concatenate([cases[i]["X"] for i in group])
        at, tasks = 0, []
        for i in group:
            c, n = cases[i], cases[i]["X"].shape[0]
            tasks.append((np.arange(at, at + n), c["y"], c["w"], c["seed"], c["mean"], c["scale"]))
            at += n
        for i, tree in zip(group, aT.tree_fit_regression(X, tasks).trees):
            out[i] = tree
    return out


def test_edge_cases_equal_scikit_learns_trees(gpu_lib):
    """One in-bag row, two rows with equal / distinct targets, every feature constant, a constant target, three of five features
    constant, 1 / 256 dims, integer ties, adjacent float32 values, a chain of depth 299, both signs at the magnitude bound, a row of
    weight 8191, bootstraps of 63 .. 513 rows and one over 9 dims."""
    g = golden("treefit_reg_edges.npz")
    names = [str(s) for s in g["names"]]
    cases = [golden_case(g, i) for i in range(len(names))]
    for i, tree in enumerate(fit_cases(cases)):
        assert tree["value"].shape == (tree["feature"].shape[0], 1)
        same_tree(tree, g, "c%d_" % i, names[i])


def test_the_row_limit_exactly(gpu_lib):
    g = golden("treefit_reg_limit.npz")
    c = golden_case(g, 0)
    assert c["X"].shape[0] == aT.tree_fit_geometry()[1]
    same_tree(aT.tree_fit_regression(c["X"].astype(np.float64), [task_of(c)]).trees[0], g, "c0_", "row limit")


def test_one_row_more_than_the_limit_is_refused(gpu_lib):
    n = aT.tree_fit_geometry()[1] + 1
    with pytest.raises(NotImplementedError, match="8192"):
        aT.tree_fit_regression(np.zeros((n, 2)), [(np.arange(n), np.zeros(n), None, 1, np.zeros(2), np.ones(2))])


def general_cases():
    """Gaussian targets: the sums round.  300 x 9 without and with a bootstrap, and 257 x 4 (two rows per thread in one chunk)."""
    X, y = R.general_case()
    X2, y2 = R.general_case(257, 4, seed=6)
    ones = lambda n: np.ones(n, dtype=np.int32)          # noqa: E731
    return [dict(X=X, y=y, w=ones(300), mean=np.zeros(9), scale=np.ones(9), seed=77),
            dict(X=X, y=y, w=R.bootstrap_weights(7, 300).astype(np.int32), mean=np.zeros(9), scale=np.ones(9), seed=78),
            dict(X=X2, y=y2, w=R.bootstrap_weights(8, 257).astype(np.int32), mean=X2.mean(0), scale=X2.std(0), seed=79)]


def test_same_bits_alone_and_anywhere_in_a_batch(gpu_lib):
    """With targets whose sums ROUND: the fixed order of every sum makes a tree a function of its task alone."""
    g = golden("treefit_reg_edges.npz")
    names = [str(s) for s in g["names"]]
    target = dict(general_cases()[2])
    fillers = [golden_case(g, names.index(n)) for n in ("rows_63", "rows_257", "dims_1", "both_signs_at_the_bound")]
    pad = lambda c: dict(c, X=np.pad(c["X"], ((0, 0), (0, 4 - c["X"].shape[1]))), mean=np.pad(c["mean"], (0, 4 - c["X"].shape[1])),      # noqa: E731
                         scale=np.pad(c["scale"], (0, 4 - c["X"].shape[1]), constant_values=1.0))
    alone = fit_cases([target])[0]
    batch = [pad(fillers[i % 4]) for i in range(300)]
    places = (0, 1, 137, 255, 256, 299)
    for p in places:
        batch[p] = target
    trees = fit_cases(batch)
    for p in places:
        for f in FIELDS:
            a, b = np.asarray(trees[p][f]), np.asarray(alone[f])
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (p, f)
    again = fit_cases(batch)                                                        # and from launch to launch
    assert all(np.asarray(again[i][f]).tobytes() == np.asarray(trees[i][f]).tobytes() for i in range(300) for f in FIELDS)


def test_random_exact_cases_equal_the_restatement(gpu_lib):
    rng = np.random.default_rng(3)
    cases = []
    for n, d in ((2, 3), (3, 1), (17, 12), (90, 5), (130, 2), (200, 7), (300, 12)):
        X = np.round(rng.standard_normal((n, d)) * 4) / 4                          # ties in every column
        if d > 5:
            X[:, 5] = 2.0
        y = R.eighths(rng.standard_normal(n) * 20 + 8 * X[:, 0])
        w = R.bootstrap_weights(int(rng.integers(0, 2**31)), n).astype(np.int32)
        R.assert_exact(y, w)
        cases.append(dict(X=X, y=y, w=w, mean=X.mean(0), scale=np.where(X.std(0) > 0, X.std(0), 1.0), seed=int(rng.integers(0, 2**32))))
    for c, tree in zip(cases, fit_cases(cases)):
        ref = R.fit_tree(R.standardize32(c["X"], c["mean"], c["scale"]), c["y"], c["w"], c["seed"])
        for f in FIELDS:
            a, b = np.asarray(tree[f]), np.asarray(ref[f])
            assert a.shape == b.shape and np.array_equal(a, b), (c["X"].shape, f)
            assert b.dtype.kind != "f" or a.tobytes() == b.astype(np.float64).tobytes(), (c["X"].shape, f)


def test_general_targets_give_valid_cart_trees(gpu_lib):
    """No equality to scikit-learn here: each tree is walked with exact arithmetic (candidate, near-maximal proxy, midpoint rule,
    leaves, values, counts; without bootstrap every training row is predicted as its own target)."""
    cases = general_cases()
    for c, tree in zip(cases, fit_cases(cases)):
        x32 = R.standardize32(c["X"], c["mean"], c["scale"])
        distinct = bool(np.all(c["w"] == 1))
        assert R.check_cart_tree(tree, x32, c["y"], c["w"], distinct=distinct) == int(np.count_nonzero(c["w"])) - 1


def test_nan_and_infinity_in_the_features_are_scikit_learns_errors(gpu_lib):
    X = np.random.default_rng(0).standard_normal((30, 4))
    y = np.arange(30) / 8
    for bad, text in ((np.nan, "NaN"), (np.inf, "infinity"), (1e39, "infinity")):
        Z = X.copy()
        Z[11, 2] = bad
        with pytest.raises(ValueError, match=text):
            aT.tree_fit_regression(Z, [(np.arange(30), y, None, 1, np.zeros(4), np.ones(4))])
        with pytest.raises(ValueError, match=text):
            aT.forest_regression_split_fit_predict(Z, y, [(np.arange(20), np.arange(20, 30), np.zeros(4), np.ones(4), (3, 1))])
        aT.forest_regression_split_fit_predict(Z, y, [(np.arange(10), np.arange(20, 30), np.zeros(4), np.ones(4), (3, 1))])      # the row is not used
        if bad == bad:                                                              # an infinite TEST value
            with pytest.raises(ValueError, match=text):
                aT.forest_regression_split_fit_predict(Z, y, [(np.arange(20, 30), np.arange(5, 15), np.zeros(4), np.ones(4), (3, 1))])


def test_sweep_equals_scikit_learns_forests(gpu_lib):
    """n_estimators 1 .. 7 over six jobs, one with a single test row: test and training predictions, bit for bit."""
    g = golden("treefit_reg_sweep.npz")
    X, y, jobs = R.sweep_case()
    res = aT.forest_regression_split_fit_predict(X, y, jobs, train_pred=True)
    assert res.pred.shape == (sum(len(j[1]) for j in jobs),) and res.train_pred.shape == (sum(len(j[0]) for j in jobs),) and res.n_chunks == 1
    for j in range(len(jobs)):
        pred, train_pred = res.job(j)
        for got, want in ((pred, g["j%d_pred" % j]), (train_pred, g["j%d_train_pred" % j])):
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), j
    plain = aT.forest_regression_split_fit_predict(X, y, jobs)
    assert plain.train_pred is None and plain.pred.tobytes() == res.pred.tobytes()
    no_test = aT.forest_regression_split_fit_predict(X, y, [(j[0], j[1][:0]) + j[2:] for j in jobs[:2]], train_pred=True)
    assert no_test.pred.shape == (0,) and no_test.train_pred.tobytes() == res.train_pred[:360].tobytes()
    try:
        import sklearn
    except ImportError:
        return
    if sklearn.__version__ != str(g["sklearn_version"]):
        return                                                                      # the goldens are the recorded version's
    for j in (0, 4, 5):
        pred, train_pred, _ = R.sklearn_forest(X, y, jobs[j])
        assert np.array_equal(res.job(j)[0], pred) and np.array_equal(res.job(j)[1], train_pred)


def test_train_random_forest_regression_device_equals_scikit_learns_fit(gpu_lib):
    sklearn_ensemble = live_sklearn() and pytest.importorskip("sklearn.ensemble")
    X, y, jobs = R.sweep_case()
    m = sklearn_ensemble.RandomForestRegressor(n_estimators=12, random_state=21).fit(X, y)
    want = aT.forest_arrays(m)
    got, train_error = aT.train_random_forest_regression_device(X, y, 12, random_state=21)
    assert got.kind == "regressor" and got.n_dims == X.shape[1]
    for f in ("node_offsets", "children_left", "children_right", "feature", "threshold", "missing_go_to_left", "value"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f
    for f in ("impurity", "n_node_samples", "weighted_n_node_samples"):
        assert np.array_equal(getattr(got, f), np.concatenate([getattr(e.tree_, f) for e in m.estimators_])), f
    assert train_error == np.mean(np.abs(m.predict(X) - y))
    np.random.seed(21)                                                              # random_state=None: NumPy's global state, as scikit-learn
    again, _ = aT.train_random_forest_regression_device(X, y, 12)
    assert again.threshold.tobytes() == got.threshold.tobytes() and np.random.randint(1000) == _after(21, 12)      # twelve draws, no more
    Z = np.random.default_rng(1).standard_normal((40, X.shape[1]))
    zeros, ones = np.zeros(X.shape[1]), np.ones(X.shape[1])
    assert np.array_equal(aT.regress([got], "randomforest", Z.T, zeros, ones)[0], m.predict(Z))          # every regressor reader takes it
    assert aT.regression_wrapper(got, "randomforest", Z[3]) == m.predict(Z[3:4])[0]
    back = aT.to_sklearn_forest_regressor(got)
    assert np.array_equal(back.predict(Z), m.predict(Z))


def test_evaluate_regression_device_equals_scikit_learn_on_the_same_splits(gpu_lib):
    """Exact targets: the return value and the printed table are what scikit-learn's forests give for the same permutations and seeds."""
    sklearn_ensemble = live_sklearn() and pytest.importorskip("sklearn.ensemble")
    from sklearn.preprocessing import StandardScaler
    X, y, _ = R.sweep_case()
    X, y = X[:90] * 3.0 + 1.0, y[:90]
    params, n_exp, n, n_train = [2, 5, 9], 3, 90, 81
    Z = StandardScaler().fit_transform(X)
    np.random.seed(31)                      # the device mode's order of draws: every permutation, parameter-major, then one seed per job
    perms = [[np.random.permutation(range(n)) for _ in range(n_exp)] for _ in params]
    seeds = [[int(np.random.randint(np.iinfo(np.int32).max)) for _ in range(n_exp)] for _ in params]
    state_after = np.random.get_state()[1].copy()
    errs, train_errs, base_errs = [], [], []
    for p, prow, srow in zip(params, perms, seeds):
        e, t, b = [], [], []
        for perm, seed in zip(prow, srow):
            tr, te = perm[:n_train], perm[n_train:]
            m = sklearn_ensemble.RandomForestRegressor(n_estimators=p, random_state=seed).fit(Z[tr], y[tr])
            pred, base = m.predict(Z[te]), np.mean([y[i] for i in tr])
            e.append(np.array([(pred[k] - y[i]) * (pred[k] - y[i]) for k, i in enumerate(te)]).mean())
            b.append(np.array([(base - y[i]) * (base - y[i]) for i in te]).mean())
            t.append(np.mean(np.abs(m.predict(Z[tr]) - y[tr])))
        errs.append(np.array(e).mean())
        train_errs.append(np.array(t).mean())
        base_errs.append(np.array(b).mean())
    best = int(np.argmin(errs))
    np.random.seed(31)
    ret, text = _run(aT.evaluate_regression, X, y, n_exp, "randomforest", params, forest_fit="device")
    assert ret == (params[best], errs[best], base_errs[best])
    assert np.array_equal(np.random.get_state()[1], state_after)
    lines = text.splitlines()
    assert lines[0].split() == ["Param", "MSE", "T-MSE", "R-MSE"] and len(lines) == 1 + len(params)
    for i, line in enumerate(lines[1:]):
        assert line.split()[:4] == ["%.4f" % params[i], "%.2f" % errs[i], "%.2f" % train_errs[i], "%.2f" % base_errs[i]]
        assert line.rstrip().endswith("best") == (i == best)


def test_evaluate_regression_default_mode_is_unchanged(gpu_lib):
    """forest_fit="sklearn" (and no keyword at all): scikit-learn's fits in the parent's loop, consuming the global state as before
    (every permutation followed by its forest's own draws)."""
    sklearn_ensemble = live_sklearn() and pytest.importorskip("sklearn.ensemble")
    from sklearn.preprocessing import StandardScaler
    X, y, _ = R.sweep_case()
    X, y = X[:60], y[:60]
    params, n_exp, n, n_train = [2, 4], 2, 60, 54
    Z = StandardScaler().fit_transform(X)
    np.random.seed(14)
    errs, base_errs = [], []
    for p in params:
        e, b = [], []
        for _ in range(n_exp):
            perm = np.random.permutation(range(n))
            tr, te = perm[:n_train], perm[n_train:]
            m = sklearn_ensemble.RandomForestRegressor(n_estimators=p).fit(Z[tr], [y[i] for i in tr])
            pred, base = m.predict(Z[te]), np.mean([y[i] for i in tr])
            e.append(np.array([(pred[k] - y[i]) * (pred[k] - y[i]) for k, i in enumerate(te)]).mean())
            b.append(np.array([(base - y[i]) * (base - y[i]) for i in te]).mean())
        errs.append(np.array(e).mean())
        base_errs.append(np.array(b).mean())
    state_after = np.random.get_state()[1].copy()
    best = int(np.argmin(errs))
    for kw in (dict(forest_fit="sklearn"), dict()):
        np.random.seed(14)
        ret, text = _run(aT.evaluate_regression, X, y, n_exp, "randomforest", params, **kw)
        assert ret == (params[best], errs[best], base_errs[best]) and "best" in text
        assert np.array_equal(np.random.get_state()[1], state_after)


def test_feature_extraction_train_regression_forest_fit_device(gpu_lib, tmp_path):
    """A tiny folder of synthetic clips and one CSV of targets: the model file is a pickled RandomForestRegressor with its MEANS file,
    loads through load_model(..., is_regression=True), and file_regression runs on it."""
    sklearn_ensemble = pytest.importorskip("sklearn.ensemble")
    import scipy.io.wavfile as wavfile
    import train_ref
    g = train_ref.load_golden("train_dir_small")
    folder = str(tmp_path / "clips")
    os.makedirs(folder)
    names = ["t%02d.wav" % i for i in range(6)] + ["b%02d.wav" % i for i in range(6)]
    for name in names:
        wavfile.write(os.path.join(folder, name), int(g["fs"]), g["wav_x_%s/%s" % ("tones" if name[0] == "t" else "bursts", name)])
    with open(os.path.join(folder, "level.csv"), "wt") as fo:
        for i, name in enumerate(names):
            fo.write("%s,%s\n" % (name, (i % 6) / 8 + (2.0 if name[0] == "b" else 0.0)))
    model = str(tmp_path / "reg")
    np.random.seed(5)
    (errors, base_errors, best), text = _run(aT.feature_extraction_train_regression, folder, float(g["mid_window"]), float(g["mid_step"]),
                                             float(g["short_window"]), float(g["short_step"]), "randomforest", model, forest_fit="device")
    assert len(errors) == len(base_errors) == 1 and best[0] in (5, 10, 25, 50, 100) and "Regression task level" in text
    loaded = aT.load_model(model + "_level", is_regression=True)
    assert type(loaded[0]) is sklearn_ensemble.RandomForestRegressor and len(loaded[0].estimators_) == best[0] and len(loaded[1]) == 136
    arrays = aT.forest_arrays(loaded[0])
    Z = np.random.default_rng(2).standard_normal((25, 136))
    assert np.array_equal(aT.regress([arrays], "randomforest", Z.T, np.zeros(136), np.ones(136))[0], loaded[0].predict(Z))
    values, tasks = aT.file_regression(os.path.join(folder, "b03.wav"), model, "randomforest")
    assert tasks == ["level"] and len(values) == 1 and 0.0 <= values[0] <= 2.625
