"""GPU checks of the gradient-boosting fit: the Friedman instance of tree_fit_kernel alone (paa_tree_fit_boost_tasks_f64 /
audioTrainTest.tree_fit_boosting), the staged sweep (paa_boost_fit_splits_f64 / boosting_split_fit_predict: boost_gradient_kernel, the
trees with their Newton leaf steps, the boosted predict kernels) and the public path (evaluate_classifier(boosting_fit="device"),
train_gradient_boosting_device, to_sklearn_boosting, extract_features_and_train(boosting_fit="device")).
Acceptances, as the contract of DESIGN section 4 K20 has them: EQUALITY with scikit-learn 1.7.2 (goldens made from the live package)
where every sum is exact -- the builder's cases with targets in eighths, stage 0 of balanced 2-, 4- and 8-class jobs; train_score_ and
the training raw predictions within 1e-9 relative for whole fits; a traced replay on the host that is independent of scikit-learn;
and the same bits alone, in a batch and across chunks."""
import os
from fractions import Fraction

import numpy as np
import pytest

import boost_edge_cases as E
import boost_ref as B
import train_ref
from pyaudioanalysis_amd import audioTrainTest as aT
from test_boost_cpu import FIELDS, builder_golden, golden, rel, same_tree, stage0_golden, whole_golden
from test_boost_edges_ref_cpu import whole_golden as edge_whole_golden

pytestmark = pytest.mark.gpu


def task_of(c):
    return (np.arange(c["X"].shape[0]), c["y"], c["w"], c["seed"], c["mean"], c["scale"])


def whole_job(X, tr, te, stages, rs):
    d = X.shape[1]
    return (tr, te, np.zeros(d), np.ones(d), (stages, rs))


def test_builder_equals_scikit_learns_trees(gpu_lib):
    """Builder alone, exact targets: one row, two rows equal / distinct, a constant target, every feature constant, ties in every column,
    adjacent float32 values, 1 and 256 dims, depths 1, 2, 3 and 12, a depth limit reached with impure rows, 63 .. 513 rows."""
    cases, g = builder_golden()
    names = [n for n in cases if n != "row_limit"]
    for depth in sorted({cases[n]["max_depth"] for n in names}):
        for d in sorted({cases[n]["X"].shape[1] for n in names if cases[n]["max_depth"] == depth}):
            group = [n for n in names if cases[n]["max_depth"] == depth and cases[n]["X"].shape[1] == d]
            X = np.concatenate([cases[n]["X"] for n in group])
            at, tasks = 0, []
            for n in group:
                c = cases[n]
                tasks.append((np.arange(at, at + c["X"].shape[0]), c["y"], c["w"], c["seed"], c["mean"], c["scale"]))
                at += c["X"].shape[0]
            for n, tree in zip(group, aT.tree_fit_boosting(X, tasks, max_depth=depth).trees):
                assert tree["value"].shape == (tree["feature"].shape[0], 1)
                same_tree(tree, g, "c%d_" % list(cases).index(n), n)
    limited = cases["impure_at_the_limit"]
    assert g["c%d_impurity" % list(cases).index("impure_at_the_limit")][-1] > 1.0 and limited["max_depth"] == 2       # an impure leaf at the limit


def test_builder_at_the_row_limit(gpu_lib):
    """8192 rows x 3 dims: the LDS peak of the instance."""
    cases, g = builder_golden()
    c = cases["row_limit"]
    assert c["X"].shape[0] == aT.tree_fit_geometry()[1]
    same_tree(aT.tree_fit_boosting(c["X"], [task_of(c)], max_depth=c["max_depth"]).trees[0], g, "c%d_" % list(cases).index("row_limit"), "row limit")


def test_builder_with_gaussian_targets_builds_valid_trees(gpu_lib):
    for name, c in B.gaussian_cases().items():
        tree = aT.tree_fit_boosting(c["X"], [task_of(c)], max_depth=3).trees[0]
        internal = B.check_boost_stage(tree, B.standardize32(c["X"], c["mean"], c["scale"]), c["y"], c["w"], 3)
        assert internal == 7, (name, internal)
        again = aT.tree_fit_boosting(c["X"], [task_of(c), task_of(c)], max_depth=3).trees[1]
        for f in FIELDS:
            assert again[f].tobytes() == tree[f].tobytes(), (name, f)


def model_trees(m):
    """A boosted ForestArrays as a list of tree dicts."""
    out = []
    for t in range(m.node_offsets.shape[0] - 1):
        lo, hi = int(m.node_offsets[t]), int(m.node_offsets[t + 1])
        tree = {f: getattr(m, f)[lo:hi] for f in FIELDS if f != "value"}
        tree["value"] = m.value[lo:hi].reshape(-1, 1)
        out.append(tree)
    return out


@pytest.mark.parametrize("name", list(B.STAGE0))
def test_stage_0_of_balanced_jobs_equals_scikit_learn(gpu_lib, name):
    """Tree arrays AND Newton leaf values bit-equal to the live fit's, and with them init, train_score_ to the gate, raw exactly."""
    g, p, X, y, K, rs = stage0_golden(name)
    res = aT.boosting_split_fit_predict(X, y, [whole_job(X, np.arange(len(y)), np.zeros(0, dtype=int), 1, rs)], train_score=True, trees=True)
    m = res.models[0]
    assert np.array_equal(m.init, g[p + "init"]) and np.array_equal(res.train_raw[0], g[p + "train_raw"])
    assert rel(res.train_score[0], g[p + "train_score"]) <= 1e-9
    trees = model_trees(m)
    assert len(trees) == (1 if K == 2 else K)
    for t, tree in enumerate(trees):
        lo, hi = int(g[p + "node_offsets"][t]), int(g[p + "node_offsets"][t + 1])
        for f in FIELDS:
            want = g[p + f][lo:hi]
            assert np.asarray(tree[f]).reshape(-1).astype(want.dtype).tobytes() == want.tobytes(), (name, t, f)


_FITS = {}
# the whole fits: boost_ref.WHOLE (at most 240 training rows: one row per thread) and boost_edge_cases.WHOLE (600 and 777 rows; 63 classes)
WHOLE_NAMES = list(B.WHOLE) + list(E.WHOLE)


def whole_fit(name):
    """The device's fit of a whole case, once per session: (golden, prefix, X, y, tr, te, K, stages, rs, the result)."""
    if name not in _FITS:
        g, p, X, y, tr, te, K, stages, rs = (edge_whole_golden if name in E.WHOLE else whole_golden)(name)
        res = aT.boosting_split_fit_predict(X, y, [whole_job(X, tr, te, stages, rs)], proba=True, train_score=True, trees=True)
        _FITS[name] = (g, p, X, y, tr, te, K, stages, rs, res)
    return _FITS[name]


@pytest.mark.parametrize("name", WHOLE_NAMES)
def test_whole_fits_against_scikit_learn(gpu_lib, name):
    g, p, X, y, tr, te, K, stages, rs, res = whole_fit(name)
    score, raw = rel(res.train_score[0], g[p + "train_score"]), rel(res.train_raw[0], g[p + "train_raw"])
    print("%s: train_score_ within %.3g, training raw predictions within %.3g (relative)" % (name, score, raw))
    assert res.train_score[0].shape == (stages,) and res.train_raw[0].shape == g[p + "train_raw"].shape
    assert score <= 1e-9 and raw <= 1e-9


@pytest.mark.parametrize("name", WHOLE_NAMES)
def test_gradients_agree_with_the_host_to_4_ulp_of_1(gpu_lib, name):
    """Element by element, stage by stage: ONE call fits the case with 1 .. S stages (the same seed: the first s stages of every job are
    the same model, and a model is a function of its job alone); job s returns the negative gradients its last stage was fitted to, which
    boost_gradient_kernel formed from the raw predictions after s - 1 stages -- job s - 1's train_raw, the init for s = 1.  The host
    forms them from those same raw predictions with libm; they agree to 4 x 2^-52."""
    g, p, X, y, tr, te, K, stages, rs, whole = whole_fit(name)
    none = np.zeros(0, dtype=np.int64)
    res = aT.boosting_split_fit_predict(X, y, [whole_job(X, tr, none, s, rs) for s in range(1, stages + 1)], train_score=True)
    assert res.train_raw[-1].tobytes() == whole.train_raw[0].tobytes() and res.train_resid[-1].shape == res.train_raw[-1].shape
    raw = np.tile(whole.models[0].init, (len(tr), 1))
    worst = 0.0
    for s in range(stages):
        want, loss = B.gradient_and_loss(raw, y[tr], K)
        worst = max(worst, float(np.max(np.abs(res.train_resid[s] - want))))
        if s:
            assert abs(loss - res.train_score[s][s - 1]) <= 1e-12 * abs(loss) and res.train_score[s][s - 1] == whole.train_score[0][s - 1]
        raw = res.train_raw[s]
    print("%s: the device's gradients within %.3g of the host's (%.2f ulp of 1)" % (name, worst, worst * 2.0 ** 52))
    assert worst <= 4 * 2.0 ** -52


@pytest.mark.parametrize("name", WHOLE_NAMES)
def test_traced_replay_on_the_host(gpu_lib, name):
    """Independent of scikit-learn: replay the fit stage by stage from the device's own trees.  With the gradients held to 4 ulp of 1 (the
    test above), every tree a valid stage tree for the host gradients (bounds widened by that error), every leaf value within the bound derived from the sums
    (n 2^-52 sum |terms| on numerator and denominator, through the quotient), the final raw predictions to 1e-10."""
    g, p, X, y, tr, te, K, stages, rs, res = whole_fit(name)
    m = res.models[0]
    trees = model_trees(m)
    k_out = 1 if K == 2 else K
    x32, yt = X[tr].astype(np.float32), y[tr]
    n = len(tr)
    ones = np.ones(n, dtype=np.int64)
    raw = np.tile(m.init, (n, 1))
    g_err = 4 * 2.0 ** -52
    u = 2.0 ** -52
    for s in range(stages):
        resid, loss = B.gradient_and_loss(raw, yt, K)
        if s:
            assert abs(loss - res.train_score[0][s - 1]) <= 1e-10 * abs(loss)
        for k in range(k_out):
            tree = trees[s * k_out + k]
            B.check_boost_stage(tree, x32, resid[:, k], ones, B.MAX_DEPTH, y_err=g_err)
            yk = (yt == (1 if K == 2 else k)).astype(np.float64)
            node_of = np.zeros(n, dtype=np.int64)
            for i in range(n):
                node = 0
                while tree["children_left"][node] >= 0:
                    node = tree["children_left"][node] if np.float64(x32[i, tree["feature"][node]]) <= tree["threshold"][node] else tree["children_right"][node]
                node_of[i] = node
            for node in np.flatnonzero(tree["children_left"] < 0):
                rows = np.flatnonzero(node_of == node)
                nn = len(rows)
                r, pr = resid[rows, k], yk[rows] - resid[rows, k]
                num, den = float(sum(Fraction(float(v)) for v in r)), float(sum(Fraction(float(v)) for v in pr * (1.0 - pr)))
                e_num = nn * u * np.abs(r).sum() + nn * g_err                     # the summation order, the gradients' own error
                e_den = nn * u * np.abs(pr * (1.0 - pr)).sum() + 2 * nn * g_err
                factor = 1.0 if K == 2 else (K - 1) / K
                got = float(tree["value"][node, 0])
                if abs(den) / nn < 1e-150:
                    assert got == 0.0
                    continue
                want = factor * num / den
                bound = (factor * e_num + abs(want) * e_den) / (abs(den) - e_den) + 8 * u * abs(want)
                assert abs(got - want) <= bound, (name, s, k, node, got, want, bound)
                raw[rows, k] = raw[rows, k] + B.LEARNING_RATE * got
    assert np.max(np.abs(raw - res.train_raw[0])) <= 1e-10
    assert abs(B.gradient_and_loss(raw, yt, K)[1] - res.train_score[0][-1]) <= 1e-10 * abs(res.train_score[0][-1])


@pytest.mark.parametrize("name", WHOLE_NAMES)
def test_held_out_rows_are_scored_as_the_model_scores_them(gpu_lib, name):
    """Labels and probabilities of the sweep equal to_sklearn_boosting(model).predict / predict_proba within 1e-14 (the bound of
    test_forest_gpu.py for boosted models) -- not scikit-learn's own fit, whose held-out labels move with splits that part the training
    rows identically."""
    pytest.importorskip("sklearn")
    g, p, X, y, tr, te, K, stages, rs, res = whole_fit(name)
    gb = aT.to_sklearn_boosting(res.models[0])
    labels, proba = res.job(0)
    want = gb.predict_proba(X[te].astype(np.float32))
    assert proba.shape == want.shape and np.max(np.abs(proba - want)) <= 1e-14
    assert np.array_equal(labels, gb.predict(X[te].astype(np.float32)))          # every held-out row
    assert np.max(np.abs(gb._raw_predict(X[tr].astype(np.float32)) - res.train_raw[0])) <= 1e-14 * max(1.0, np.max(np.abs(res.train_raw[0])))
    assert np.array_equal(gb.train_score_, res.train_score[0])


def batch_jobs():
    """Jobs with 1, 3 and 2 stages and 2, 3 and 8 classes over one matrix of 12 dims."""
    parts, jobs, at = [], [], 0
    ys = []
    for name, stages in (("fit_2x150x5", 1), ("fit_3x150x9_unbalanced", 3), ("fit_8x240x12", 2)):
        X, y, tr, te, K, _, rs = B.whole_case(name)
        Xp = np.zeros((X.shape[0], 12))
        Xp[:, :X.shape[1]] = X
        Xp[:, X.shape[1]:] = np.random.RandomState(K).randn(X.shape[0], 12 - X.shape[1]).astype(np.float32)
        parts.append(Xp)
        ys.append(y + 10 * len(jobs))                                               # other class VALUES per job
        jobs.append((tr + at, te + at, Xp[tr].mean(0), Xp[tr].std(0), (stages, rs)))
        at += X.shape[0]
    return np.concatenate(parts), np.concatenate(ys), jobs


def result_bytes(res, j):
    m = res.models[j]
    return b"".join([res.job(j)[0].tobytes(), res.job(j)[1].tobytes(), res.train_score[j].tobytes(), res.train_raw[j].tobytes(), m.init.tobytes()] +
                    [np.ascontiguousarray(getattr(m, f)).tobytes() for f in FIELDS] + [m.node_offsets.tobytes()])


def test_same_bits_alone_in_a_batch_and_across_chunks(gpu_lib):
    X, y, jobs = batch_jobs()
    both = aT.boosting_split_fit_predict(X, y, jobs, proba=True, train_score=True, trees=True)
    again = aT.boosting_split_fit_predict(X, y, jobs, proba=True, train_score=True, trees=True)
    assert both.n_chunks == 1 and [len(c) for c in both.classes] == [2, 3, 8] and both.classes[1].tolist() == [10, 11, 12]
    assert set(both.job(2)[0].tolist()) <= set(range(20, 28))
    for j in range(3):
        alone = aT.boosting_split_fit_predict(X, y, [jobs[j]], proba=True, train_score=True, trees=True)
        assert result_bytes(alone, 0) == result_bytes(both, j) == result_bytes(again, j), j
        assert both.models[j].node_offsets.shape[0] - 1 == jobs[j][4][0] * (1 if len(both.classes[j]) == 2 else len(both.classes[j]))
    # two chunks: a bound that holds the largest job (a job is never cut) but not all three
    chunked = aT.boosting_split_fit_predict(X, y, jobs, proba=True, train_score=True, trees=True, chunk_bytes=96 * 1024)
    assert chunked.n_chunks >= 2
    for j in range(3):
        assert result_bytes(chunked, j) == result_bytes(both, j), j


def test_evaluate_classifier_boosting_fit_device(gpu_lib):
    pytest.importorskip("sklearn")
    from sklearn.preprocessing import StandardScaler
    from test_train_gpu import _run
    feats = train_ref.three_class_features()
    names, params, n_exp = ["a", "b", "c"], [2, 4], 2
    X, y = aT.features_to_matrix(feats)
    np.random.seed(17)                      # the device mode's order of draws: every split, parameter-major, then one seed per job
    splits = [[aT._draw_split(X.shape[0], 0.9) for _ in range(n_exp)] for _ in params]
    seeds = [[int(np.random.randint(np.iinfo(np.int32).max)) for _ in range(n_exp)] for _ in params]
    jobs = []
    for prm, row, srow in zip(params, splits, seeds):
        for (tr, te), seed in zip(row, srow):
            sc = StandardScaler().fit(X[tr])
            jobs.append((tr, te, sc.mean_, sc.scale_, (prm, seed)))
    want = aT.boosting_split_fit_predict(X, y, jobs)
    np.random.seed(17)
    (ret, cms, preds), text = _run(aT.evaluate_classifier_full, feats, names, "gradientboosting", params, 0, n_exp=n_exp, boosting_fit="device")
    assert ret in params and "best Acc" in text
    assert np.array_equal(np.concatenate([p for row in preds for p in row]), want.label.astype(np.float64))
    np.random.seed(17)
    assert _run(aT.evaluate_classifier, feats, names, "gradientboosting", params, 0, n_exp=n_exp, boosting_fit="device")[0] == ret


def test_train_device_and_to_sklearn_boosting(gpu_lib):
    sklearn_ensemble = pytest.importorskip("sklearn.ensemble")
    import pickle
    X, y, tr, te, K, stages, rs = B.whole_case("fit_3x150x9_unbalanced")
    m = aT.train_gradient_boosting_device(X[tr], y[tr] * 2.0 + 1.0, 4, random_state=rs)             # class VALUES 1, 3, 5
    assert m.kind == "boosted" and m.classes_.tolist() == [1.0, 3.0, 5.0] and m.train_score_.shape == (4,) and m.node_offsets.shape == (13,)
    gb = pickle.loads(pickle.dumps(aT.to_sklearn_boosting(m)))
    assert type(gb) is sklearn_ensemble.GradientBoostingClassifier and gb.estimators_.shape == (4, 3) and gb.n_trees_per_iteration_ == 3
    labels, proba = aT.forest_predict(m, X[te].T, np.zeros(9), np.ones(9))
    assert np.max(np.abs(proba - gb.predict_proba(X[te]))) <= 1e-14 and set(labels.tolist()) <= {1.0, 3.0, 5.0}
    assert aT.classifier_wrapper(gb, "gradientboosting", X[te][0])[0] == aT.classifier_wrapper(m, "gradientboosting", X[te][0])[0]


def test_extract_features_and_train_boosting_fit_device(gpu_lib, tmp_path):
    """The model file is a pickled GradientBoostingClassifier with the MEANS file beside it; load_model and file_classification read it."""
    sklearn_ensemble = pytest.importorskip("sklearn.ensemble")
    from test_train_gpu import _run, _write_dir
    g = train_ref.load_golden("train_dir_small")
    paths = _write_dir(g, str(tmp_path))
    model = str(tmp_path / "model_gb")
    np.random.seed(int(g["seed"]))
    _run(aT.extract_features_and_train, paths, float(g["mid_window"]), float(g["mid_step"]), float(g["short_window"]),
         float(g["short_step"]), "gradientboosting", model, boosting_fit="device")
    loaded = aT.load_model(model)
    assert len(loaded) == 9 and loaded[3] == ["tones", "bursts"] and loaded[1].shape == (136,)
    assert type(loaded[0]) is sklearn_ensemble.GradientBoostingClassifier and loaded[0].classes_.tolist() == [0.0, 1.0]
    assert loaded[0].estimators_.shape[0] in (10, 25, 50, 100, 200, 500) and loaded[0].train_score_.shape == (loaded[0].estimators_.shape[0],)
    for wav, want in (("tones/t03.wav", "tones"), ("bursts/b07.wav", "bursts")):
        class_id, P, names = aT.file_classification(os.path.join(str(tmp_path), wav), model, "gradientboosting")
        assert names[int(class_id)] == want and P.shape == (2,) and abs(P.sum() - 1.0) < 1e-9


def test_refusals_on_the_device(gpu_lib):
    n = aT.tree_fit_geometry()[1] + 1
    job = lambda X, k=1: (np.arange(X.shape[0]), np.arange(2), np.zeros(X.shape[1]), np.ones(X.shape[1]), (k, 1))       # noqa: E731
    with pytest.raises(NotImplementedError, match="8192"):
        aT.boosting_split_fit_predict(np.zeros((n, 2)), np.arange(n) % 2, [job(np.zeros((n, 2)))])
    with pytest.raises(NotImplementedError, match="8192"):
        aT.tree_fit_boosting(np.zeros((n, 2)), [(np.arange(n), np.zeros(n), None, 1, np.zeros(2), np.ones(2))])
    X = np.random.RandomState(3).randn(40, 3)
    y = np.arange(40) % 2
    for bad, msg in ((np.nan, "Input X contains NaN."), (np.inf, "Input X contains infinity")):
        Xb = X.copy()
        Xb[5, 1] = bad
        with pytest.raises(ValueError, match=msg):
            aT.boosting_split_fit_predict(Xb, y, [job(Xb)])
        with pytest.raises(ValueError, match=msg):
            aT.tree_fit_boosting(Xb, [(np.arange(40), y.astype(float), None, 1, np.zeros(3), np.ones(3))])
    Xb = X.copy()
    Xb[0, 0] = 1e39                                                                 # finite in FP64, infinite in float32
    with pytest.raises(ValueError, match="infinity"):
        aT.boosting_split_fit_predict(Xb, y, [job(Xb)])
