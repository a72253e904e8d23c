"""GPU checks of the tree builder (tree_fit_kernel through paa_tree_fit_tasks_f64 / audioTrainTest.tree_fit), of the forest split
sweep built on it (paa_forest_fit_splits_f64 / forest_split_fit_predict, evaluate_classifier(forest_fit="device")) and of the final
fit (train_forest_device, to_sklearn_forest, extract_features_and_train(forest_fit="device")).  The acceptance is EQUALITY with
scikit-learn 1.7.2's own trees as the goldens record them (scripts/make_treefit_golden.py): integer arrays equal, float64 arrays
bit-equal; live scikit-learn is compared too where it is installed."""
import os

import numpy as np
import pytest

import train_ref
import treefit_ref as R
from pyaudioanalysis_amd import audioTrainTest as aT
from test_treefit_cpu import FIELDS, golden, golden_case, live_sklearn, same_tree

pytestmark = pytest.mark.gpu


def task_of(c):
    return (np.arange(c["X"].shape[0]), c["y"], c["w"], c["seed"], c["mean"], c["scale"])


def fit_cases(cases, splitter):
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
        for i, tree in zip(group, aT.tree_fit(X, tasks, splitter).trees):
            out[i] = tree
    return out


def test_geometry(gpu_lib):
    assert aT.tree_fit_geometry() == (256, 8192, 64, 256, 8191, 1024)


@pytest.mark.parametrize("splitter", ["best", "random"])
def test_edge_cases_equal_scikit_learns_trees(gpu_lib, splitter):
    """One in-bag row, one class, two rows, every feature constant, three of five constant, integer ties, adjacent float32 values,
    values near 3e38, weights 0 / 1 / >= 2, 63 .. 257 rows, a chain of depth ~300, 2 / 8 / 64 classes, 1 / 136 / 138 dims, a
    bootstrap at 136 dims and the extra-trees draw whose threshold equals the maximum."""
    g = golden("treefit_edges.npz")
    names = [str(s) for s in g["names"]]
    cases = [golden_case(g, i) for i in range(len(names))]
    for i, tree in enumerate(fit_cases(cases, splitter)):
        same_tree(tree, g, "c%d_%s_" % (i, splitter), names[i])


@pytest.mark.parametrize("splitter", ["best", "random"])
def test_the_row_limit_exactly(gpu_lib, splitter):
    g = golden("treefit_limit.npz")
    c = golden_case(g, 0)
    assert c["X"].shape[0] == aT.tree_fit_geometry()[1]
    same_tree(aT.tree_fit(c["X"].astype(np.float64), [task_of(c)], splitter).trees[0], g, "c0_%s_" % splitter, "row limit")


def test_one_row_more_than_the_limit_is_refused(gpu_lib):
    n = aT.tree_fit_geometry()[1] + 1
    with pytest.raises(NotImplementedError, match="8192"):
        aT.tree_fit(np.zeros((n, 2)), [(np.arange(n), np.arange(n) % 2, None, 1, np.zeros(2), np.ones(2))], "best")


@pytest.mark.parametrize("splitter", ["best", "random"])
def test_same_bits_alone_and_anywhere_in_a_batch(gpu_lib, splitter):
    g = golden("treefit_edges.npz")
    names = [str(s) for s in g["names"]]
    target = golden_case(g, names.index("weights_0_1_2"))
    fillers = [golden_case(g, names.index(n)) for n in ("rows_63", "classes_8", "integer_ties", "rows_257")]
    assert all(f["X"].shape[1] <= 6 for f in fillers)
    pad = lambda c: dict(c, X=np.pad(c["X"], ((0, 0), (0, 6 - c["X"].shape[1]))), mean=np.pad(c["mean"], (0, 6 - c["X"].shape[1])),      # noqa: E731
                         scale=np.pad(c["scale"], (0, 6 - c["X"].shape[1]), constant_values=1.0))
    alone = fit_cases([target], splitter)[0]
    same_tree(alone, g, "c%d_%s_" % (names.index("weights_0_1_2"), splitter), "alone")
    batch = [pad(fillers[i % 4]) for i in range(300)]
    places = (0, 1, 137, 255, 256, 299)
    for p in places:
        batch[p] = target
    trees = fit_cases(batch, splitter)
    for p in places:
        for f in FIELDS:
            a, b = np.asarray(trees[p][f]), np.asarray(alone[f])
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (p, f)
    again = fit_cases(batch, splitter)                                              # and from launch to launch
    assert all(np.asarray(again[i][f]).tobytes() == np.asarray(trees[i][f]).tobytes() for i in range(300) for f in FIELDS)


@pytest.mark.parametrize("splitter", ["best", "random"])
def test_random_cases_equal_the_restatement(gpu_lib, splitter):
    rng = np.random.default_rng(3)
    cases = []
    for n, k in ((2, 2), (3, 2), (17, 3), (90, 5), (130, 2), (200, 7)):
        X = np.round(rng.standard_normal((n, 7)) * 4) / 4 + rng.integers(0, k, n)[:, None] * 0.25      # ties in every column
        X[:, 5] = 2.0
        y = np.arange(n) % k
        w = rng.integers(0, 4, n).astype(np.int32)
        w[:k] = np.maximum(w[:k], 1)
        cases.append(dict(X=X, y=y, w=w, mean=X.mean(0), scale=np.where(X.std(0) > 0, X.std(0), 1.0), seed=int(rng.integers(0, 2**32))))
    for c, tree in zip(cases, fit_cases(cases, splitter)):
        k = int(np.unique(c["y"]).shape[0])
        ref = R.fit_tree(R.standardize32(c["X"], c["mean"], c["scale"]), c["y"], c["w"], k, c["seed"], splitter)
        for f in FIELDS:
            assert np.asarray(tree[f]).shape == np.asarray(ref[f]).shape and np.array_equal(tree[f], ref[f]), (c["X"].shape, f)


def test_classes_are_those_present_in_the_task(gpu_lib):
    X = np.array([[0.0], [1.0], [2.0], [3.0]])
    res = aT.tree_fit(X, [(np.arange(4), np.array([7, 3, 7, 9]), None, 5, np.zeros(1), np.ones(1))], "best")
    assert res.classes[0].tolist() == [3, 7, 9] and res.trees[0]["value"].shape[1] == 3
    assert res.trees[0]["value"][0].tolist() == [0.25, 0.5, 0.25]


@pytest.mark.parametrize("bad,text", [(np.nan, "NaN"), (np.inf, "infinity"), (1e39, "infinity")])
def test_nan_and_infinity_are_scikit_learns_errors(gpu_lib, bad, text):
    X = np.random.default_rng(0).standard_normal((30, 4))
    X[11, 2] = bad
    y = np.arange(30) % 2
    with pytest.raises(ValueError, match=text):
        aT.tree_fit(X, [(np.arange(30), y, None, 1, np.zeros(4), np.ones(4))], "best")
    job = (np.arange(20), np.arange(20, 30), np.zeros(4), np.ones(4), (3, 1))
    with pytest.raises(ValueError, match=text):
        aT.forest_split_fit_predict(X, y, [job], "extratrees")
    aT.forest_split_fit_predict(X, y, [(np.arange(10), np.arange(20, 30), np.zeros(4), np.ones(4), (3, 1))], "extratrees")      # the row is not used
    if bad != bad:
        return                                                                      # a NaN in a test row goes the node's missing-value way
    with pytest.raises(ValueError, match=text):
        aT.forest_split_fit_predict(X, y, [(np.arange(20, 30), np.arange(5, 15), np.zeros(4), np.ones(4), (3, 1))], "randomforest")


@pytest.mark.parametrize("kind", ["randomforest", "extratrees"])
def test_sweep_equals_scikit_learns_forests(gpu_lib, kind):
    """n_estimators 1, 3, 10 x 2 experiments over 3 classes and a job whose training list lacks a class: labels and probabilities."""
    g = golden("treefit_sweep.npz")
    X, y, jobs = R.sweep_case()
    res = aT.forest_split_fit_predict(X, y, jobs, kind, proba=True)
    assert res.proba.shape == (sum(len(j[1]) for j in jobs), 3) and res.n_chunks == 1
    for j in range(len(jobs)):
        label, proba = res.job(j)
        want = g["j%d_%s_proba" % (j, kind)]
        assert np.array_equal(label, g["j%d_%s_label" % (j, kind)]), j
        assert proba.shape == want.shape and proba.tobytes() == want.tobytes(), j
    assert res.classes[6].tolist() == [0, 1] and np.all(res.proba[res._rows(6), 2] == 0.0)
    assert np.array_equal(aT.forest_split_fit_predict(X, y, jobs, kind).label, res.label)
    try:
        import sklearn
    except ImportError:
        return
    if sklearn.__version__ != str(g["sklearn_version"]):
        return                                                                      # the goldens are the recorded version's
    for j in (0, 3, 5, 6):
        label, proba, _ = R.sklearn_forest(X, y, jobs[j], kind)
        assert np.array_equal(res.job(j)[0], label) and np.array_equal(res.job(j)[1], proba)


@pytest.mark.parametrize("kind", ["randomforest", "extratrees"])
def test_train_forest_device_equals_scikit_learns_fit(gpu_lib, kind):
    sklearn_ensemble = live_sklearn() and pytest.importorskip("sklearn.ensemble")
    X, y, jobs = R.sweep_case()
    cls = sklearn_ensemble.RandomForestClassifier if kind == "randomforest" else sklearn_ensemble.ExtraTreesClassifier
    m = cls(n_estimators=12, random_state=21).fit(X, y)
    want = aT.forest_arrays(m)
    got = aT.train_forest_device(X, y, 12, kind, random_state=21)
    assert got.kind == "averaged" and got.classes_.tolist() == [0.0, 1.0, 2.0] and got.n_dims == X.shape[1]
    for f in ("node_offsets", "children_left", "children_right", "feature", "threshold", "missing_go_to_left", "value"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f
    for f in ("impurity", "n_node_samples", "weighted_n_node_samples"):
        assert np.array_equal(getattr(got, f), np.concatenate([getattr(e.tree_, f) for e in m.estimators_])), f
    np.random.seed(21)                                                              # random_state=None: NumPy's global state, as scikit-learn
    again = aT.train_forest_device(X, y, 12, kind)
    assert again.threshold.tobytes() == got.threshold.tobytes() and np.random.randint(1000) == _after(21, 12)      # twelve draws, no more
    Z = np.random.default_rng(1).standard_normal((40, X.shape[1]))
    labels, proba = aT.forest_predict(got, Z.T, np.zeros(X.shape[1]), np.ones(X.shape[1]))          # every forest reader takes it
    assert np.array_equal(labels, m.predict(Z)) and np.array_equal(proba, m.predict_proba(Z))
    back = aT.to_sklearn_forest(got, kind)
    assert np.array_equal(back.predict_proba(Z), m.predict_proba(Z))


def _after(seed, n_draws):
    """What np.random.randint(1000) gives after n_draws tree seeds were drawn from the global state seeded with `seed`."""
    rs = np.random.RandomState(seed)
    rs.randint(np.iinfo(np.int32).max, size=n_draws)
    return int(rs.randint(1000))


@pytest.mark.parametrize("kind", ["randomforest", "extratrees"])
def test_evaluate_classifier_device_equals_scikit_learn_on_the_same_splits(gpu_lib, kind):
    sklearn_ensemble = live_sklearn() and pytest.importorskip("sklearn.ensemble")
    import sklearn.metrics
    from sklearn.preprocessing import StandardScaler
    from test_train_gpu import _run
    feats = train_ref.three_class_features()
    names, params, n_exp, pct = ["a", "b", "c"], [2, 5, 10], 3, 0.8
    X, y = aT.features_to_matrix(feats)
    cls = sklearn_ensemble.RandomForestClassifier if kind == "randomforest" else sklearn_ensemble.ExtraTreesClassifier
    np.random.seed(31)                      # the device mode's order of draws: every split, parameter-major, then one seed per job
    splits = [[aT._draw_split(X.shape[0], pct) for _ in range(n_exp)] for _ in params]
    seeds = [[int(np.random.randint(np.iinfo(np.int32).max)) for _ in range(n_exp)] for _ in params]
    want_preds, want_cms = [], []
    for p, row, srow in zip(params, splits, seeds):
        cm = np.zeros((3, 3))
        for (tr, te), seed in zip(row, srow):
            scaler = StandardScaler().fit(X[tr])
            pred = cls(n_estimators=p, random_state=seed).fit(scaler.transform(X[tr]), y[tr]).predict(scaler.transform(X[te]))
            want_preds.append(pred)
            cm = cm + sklearn.metrics.confusion_matrix(y[te], pred, labels=[0, 1, 2])
        want_cms.append(cm + 0.0000000010)
    np.random.seed(31)
    (ret, cms, preds), text = _run(aT.evaluate_classifier_full, feats, names, kind, params, 0, None, n_exp=n_exp, train_percentage=pct,
                                   forest_fit="device")
    assert np.array_equal(np.concatenate([p for row in preds for p in row]), np.concatenate(want_preds))
    assert np.array_equal(np.array(cms), np.array(want_cms))
    acc = [np.trace(cm) / cm.sum() for cm in want_cms]
    assert ret == params[int(np.argmax(acc))] and "best Acc" in text
    np.random.seed(31)
    assert _run(aT.evaluate_classifier, feats, names, kind, params, 0, None, n_exp=n_exp, train_percentage=pct, forest_fit="device")[0] == ret


@pytest.mark.parametrize("kind", ["randomforest", "extratrees"])
def test_extract_features_and_train_forest_fit_device(gpu_lib, tmp_path, kind):
    """extract_features_and_train(forest_fit="device") on the train_dir_small golden's two class folders: the model file is a pickled
    scikit-learn forest with the MEANS file beside it, loads with load_model and classifies like its arrays."""
    sklearn_ensemble = pytest.importorskip("sklearn.ensemble")
    from test_train_gpu import _run, _write_dir
    g = train_ref.load_golden("train_dir_small")
    paths = _write_dir(g, str(tmp_path))
    model = str(tmp_path / ("model_" + kind))
    np.random.seed(int(g["seed"]))
    _run(aT.extract_features_and_train, paths, float(g["mid_window"]), float(g["mid_step"]), float(g["short_window"]),
         float(g["short_step"]), kind, model, forest_fit="device")
    loaded = aT.load_model(model)
    assert len(loaded) == 9 and loaded[3] == ["tones", "bursts"] and loaded[1].shape == (136,)
    cls = sklearn_ensemble.RandomForestClassifier if kind == "randomforest" else sklearn_ensemble.ExtraTreesClassifier
    assert type(loaded[0]) is cls and loaded[0].classes_.tolist() == [0.0, 1.0] and len(loaded[0].estimators_) in (10, 25, 50, 100, 200, 500)
    arrays = aT.forest_arrays(loaded[0])
    Z = np.random.default_rng(2).standard_normal((25, 136))
    labels, proba = aT.forest_predict(arrays, Z.T, np.zeros(136), np.ones(136))
    assert np.array_equal(proba, loaded[0].predict_proba(Z)) and np.array_equal(labels, loaded[0].predict(Z))
    for wav, want in (("tones/t03.wav", "tones"), ("bursts/b07.wav", "bursts")):
        class_id, P, names = aT.file_classification(os.path.join(str(tmp_path), wav), model, kind)
        assert names[int(class_id)] == want and P.shape == (2,) and abs(P.sum() - 1.0) < 1e-9
