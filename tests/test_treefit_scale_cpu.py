"""CPU-side checks of what tests/test_treefit_scale_gpu.py holds the tree builder to at its largest launch and across the chunks
of a sweep: the wide golden is the case in the tree and scikit-learn's own tree, the restatement (treefit_ref.fit_tree) equals live
scikit-learn on the dims and weight edges, the host walk and the NumPy scoring agree with scikit-learn, and the chunk rule restated
in treefit_ref.expected_chunks cuts the sweeps of the GPU tests where they are meant to be cut.  No GPU needed."""
import numpy as np
import pytest

import treefit_ref as R
import treefit_reg_ref as RR
from test_treefit_cpu import FIELDS, golden, golden_case, live_sklearn, same_tree


def test_wide_golden_is_the_case_in_the_tree():
    g = golden("treefit_wide.npz")
    c = R.wide_limit_case()
    assert str(g["kind"]) == "treefit" and list(g["names"]) == ["wide_limit_64"]
    for k, v in golden_case(g, 0).items():
        assert np.array_equal(v, c[k]), k
    w = c["w"]
    assert c["X"].shape == (8192, 3) and np.array_equal(c["X"] * 64, np.round(c["X"] * 64)) and np.array_equal(c["X"], c["X"].astype(np.float32))
    assert np.bincount(w)[[0, 1, 3, 8191]].tolist() == [400, 8192 - 701, 300, 1] and np.unique(c["y"][w > 0]).shape[0] == 64
    c32 = R.wide_limit_case(32)                                                     # the same rows, 32 classes
    assert np.array_equal(c32["X"], c["X"]) and np.array_equal(c32["w"], w) and np.array_equal(c32["y"], c["y"] % 32)
    for sp, nodes in (("best", 8089), ("random", 12351)):                           # neither trivial nor degenerate
        assert g["c0_%s_feature" % sp].shape == (nodes,) and g["c0_%s_value" % sp].shape == (nodes, 64)
        assert g["c0_%s_weighted_n_node_samples" % sp][0] == float(w.sum()) == 8192 - 701 + 900 + 8191


@pytest.mark.parametrize("splitter", ["best", "random"])
def test_wide_golden_equals_live_scikit_learn_and_passes_the_walk(splitter):
    g = golden("treefit_wide.npz")
    c = R.wide_limit_case()
    x32 = R.standardize32(c["X"], c["mean"], c["scale"])
    tree = {f: g["c0_%s_%s" % (splitter, f)] for f in FIELDS}
    assert R.check_gini_tree(tree, x32, c["y"], c["w"], 64) == (tree["feature"].shape[0] + 1) // 2
    live_sklearn()
    ref, seed = R.sklearn_tree(x32, c["y"], c["w"], 64, R.FixedSeed(c["seed"]), splitter)
    assert seed == c["seed"]
    same_tree(ref, g, "c0_%s_" % splitter, "wide limit")
    c32 = R.wide_limit_case(32)                                                     # the walk holds of scikit-learn's 32-class tree too
    ref, _ = R.sklearn_tree(x32, c32["y"], c32["w"], 32, R.FixedSeed(c32["seed"]), splitter)
    assert R.check_gini_tree(ref, x32, c32["y"], c32["w"], 32) == (ref["feature"].shape[0] + 1) // 2


def test_the_walk_refuses_wrong_trees():
    c = R.edge_cases()["weights_0_1_2"]
    x32 = R.standardize32(c["X"], c["mean"], c["scale"])
    tree = R.fit_tree(x32, c["y"], c["w"], 3, c["seed"], "best")
    R.check_gini_tree(tree, x32, c["y"], c["w"], 3)
    leaf = int(np.flatnonzero(tree["children_left"] < 0)[0])
    inner = int(np.flatnonzero(tree["children_left"] >= 0)[-1])
    for f, node, v in (("n_node_samples", leaf, tree["n_node_samples"][leaf] + 1), ("weighted_n_node_samples", inner, 1.0),
                       ("value", leaf, np.roll(tree["value"][leaf], 1)), ("impurity", inner, np.nextafter(tree["impurity"][inner], 1.0)),
                       ("threshold", 0, 1e9), ("missing_go_to_left", inner, 1 - tree["missing_go_to_left"][inner])):
        bad = {k: np.array(a, copy=True) for k, a in tree.items()}
        bad[f][node] = v
        with pytest.raises(AssertionError):
            R.check_gini_tree(bad, x32, c["y"], c["w"], 3)
    cut = {k: np.array(a, copy=True) for k, a in tree.items()}                      # an impure, splittable node made a leaf
    cut["children_left"][0] = cut["children_right"][0] = -1
    cut["feature"][0], cut["threshold"][0] = -2, -2.0
    with pytest.raises(AssertionError):
        R.check_gini_tree(cut, x32, c["y"], c["w"], 3)


@pytest.mark.parametrize("splitter", ["best", "random"])
def test_restatement_equals_live_scikit_learn_on_the_dims_and_weight_edges(splitter):
    live_sklearn()
    cases = R.dims_and_weight_cases()
    assert [c["X"].shape for c in cases.values()] == [(80, 255), (80, 256), (100, 4)]
    for name, c in cases.items():
        x32 = R.standardize32(c["X"], c["mean"], c["scale"])
        ref, seed = R.sklearn_tree(x32, c["y"], c["w"], 3, R.FixedSeed(c["seed"]), splitter)
        got = R.fit_tree(x32, c["y"], c["w"], 3, seed, splitter)
        for f in FIELDS:
            assert np.asarray(got[f]).shape == ref[f].shape and np.array_equal(got[f], ref[f]), (name, f)
        assert ref["feature"].shape[0] > 3, name


def test_score_trees_is_scikit_learns_forest_prediction():
    sklearn_ensemble = live_sklearn() and pytest.importorskip("sklearn.ensemble")
    X, y, jobs = R.sweep_case()
    tr, te, mean, scale, (ne, seed) = jobs[4]
    for cls in (sklearn_ensemble.RandomForestClassifier, sklearn_ensemble.ExtraTreesClassifier, sklearn_ensemble.RandomForestRegressor):
        m = cls(n_estimators=ne, random_state=seed).fit((X[tr] - mean) / scale, y[tr])
        trees = []
        for e in m.estimators_:
            t = {f: np.asarray(getattr(e.tree_, f)) for f in FIELDS if f != "value"}
            t["value"] = np.asarray(e.tree_.value).reshape(e.tree_.node_count, -1)
            trees.append(t)
        got = R.score_trees(trees, R.standardize32(X[te], mean, scale))
        want = m.predict_proba((X[te] - mean) / scale) if hasattr(m, "predict_proba") else m.predict((X[te] - mean) / scale).reshape(-1, 1)
        assert got.shape == want.shape and got.tobytes() == want.tobytes()


def test_expected_chunks_cuts_the_sweeps_at_interior_jobs():
    """The rule by hand: an extra-trees big job is 40 trees of 2 x 8192 - 1 nodes at 40 + 8 x 64 bytes each, 361.7 MB with its rows;
    two fit below 2^30 bytes and three do not, the tiny job rides along."""
    for kind in ("extratrees", "randomforest"):
        X, y, jobs = R.chunk_sweep_case(kind)
        assert [len(j[0]) for j in jobs] == [8192, 8192, 8192, 5, 8192, 8192, 8192] and [len(j[1]) for j in jobs] == [50, 50, 50, 7, 50, 0, 50]
        assert sorted(set(y[jobs[R.CHUNK_TINY][0]].tolist())) == [17.0, 40.0]
        assert R.expected_chunks(jobs, kind, y) == R.CHUNK_LAYOUT == [[0, 1], [2, 3, 4], [5, 6]]
        assert R.expected_chunks(jobs[:2], kind, y) == [[0, 1]] and R.expected_chunks([jobs[4]], kind, y) == [[0]]
    big = 4 * 8192 * 3 + 40 * 16383 * (40 + 8 * 64)
    assert 2 * big <= 2 ** 30 < 3 * big
    X, y, jobs = RR.chunk_sweep_case()
    assert [j[4][0] for j in jobs] == [700, 700, 700, 3, 700, 700, 700]
    assert R.expected_chunks(jobs, "regressor") == RR.CHUNK_LAYOUT
    # the small sweeps of the other tests are one chunk each, as those tests assert of the library
    X, y, jobs = R.sweep_case()
    assert R.expected_chunks(jobs, "randomforest", y) == [list(range(7))] == R.expected_chunks(jobs, "extratrees", y)
    X, labels, y, job = RR.many_test_rows_case()
    assert len(job[1]) == 32769 + 5 and np.unique(job[1]).shape[0] == len(job[1]) and R.expected_chunks([job], "regressor") == [[0]]
