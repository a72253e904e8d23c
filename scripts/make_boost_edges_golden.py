#!/usr/bin/env python3
"""Goldens of the gradient-boosting edge tests (tests/boost_edge_cases.py), from LIVE scikit-learn, beside the three files of
make_boost_golden.py, which this script does not touch:

  tests/golden/boost_edges.npz
    s<i>_   boost_edge_cases.STAGE0: balanced jobs above 256 rows (514, 1028, 8192 rows; 64 classes), GradientBoostingClassifier(
            n_estimators=1, random_state): the trees' seeds, init, every tree's arrays with its Newton leaf values, train_score_ and the
            training raw predictions.  Stage 0 is exact: the tests demand equality
    w<i>_   boost_edge_cases.WHOLE: whole fits (600 and 777 rows at 3 stages, 63 classes at 2): seeds, init, train_score_, the training raw
            predictions, predict_proba of the held-out rows
    p<i>_   boost_edge_cases.PARAMS: the 300-row job at (learning_rate, max_depth) = (1, 1), (0.5, 2), (0.1, 20): the same and every
            tree's node count
    l<i>_   boost_edge_cases.CUT_RATES: the 8-row job, init="zero", max_depth=1, one stage: train_score_ and the raw predictions, which
            land on +-2, +-18, +-33.3, +-37 and +-40
    chain<d>_  boost_edge_cases.chain_case(d), d = 20 and 21: DecisionTreeRegressor(criterion="friedman_mse", max_depth=d)
  Inputs are not stored: boost_edge_cases regenerates them from seeds and the file carries a checksum of each.

Before anything is written the NumPy restatement is compared with every record -- equality where the sums are exact, else within 1e-9
relative in the device's summation order AND in plain row order, so that no frozen case sits where two orders part (such a seed is to be
replaced).

    python scripts/make_boost_edges_golden.py        # needs scikit-learn (the golden in the tree was made with 1.7.2)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boost_edge_cases as E  # noqa: E402
import boost_ref as B  # noqa: E402
from make_boost_golden import GATE, rel, store_trees  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "boost_edges.npz")


def whole_record(store, p, what, case, learning_rate, max_depth):
    from sklearn.ensemble import GradientBoostingClassifier
    X, y, tr, te, K, stages, rs = case
    k_out = 1 if K == 2 else K
    x32 = X.astype(np.float32)
    m = GradientBoostingClassifier(n_estimators=stages, random_state=rs, learning_rate=learning_rate, max_depth=max_depth).fit(x32[tr], y[tr])
    seeds = B.tree_seeds(rs, stages * k_out)
    live_raw = m._raw_predict(x32[tr])
    trees, score, raw, init = B.fit(X[tr], y[tr], K, stages, seeds, max_depth, learning_rate)
    with E.row_order_sums():
        trees2, score2, raw2, _ = B.fit(X[tr], y[tr], K, stages, seeds, max_depth, learning_rate)
    gaps = (rel(score, m.train_score_), rel(raw, live_raw), rel(score2, m.train_score_), rel(raw2, live_raw))
    assert max(gaps) <= GATE, (what, gaps, "two summation orders part beyond the gate: replace this case's seed")
    counts = np.array([e.tree_.node_count for e in m.estimators_.ravel()], dtype=np.int64)
    assert [t["feature"].shape[0] for t in trees] == counts.tolist() == [t["feature"].shape[0] for t in trees2], what
    store.update({p + "digest": E.digest(x32, y), p + "K": np.int64(K), p + "n_stages": np.int64(stages), p + "random_state": np.int64(rs),
                  p + "seeds": np.array(seeds), p + "init": init, p + "train_score": m.train_score_, p + "train_raw": live_raw,
                  p + "test_proba": m.predict_proba(x32[te]), p + "node_count": counts, p + "learning_rate": np.float64(learning_rate),
                  p + "max_depth": np.int64(max_depth)})
    print("%-28s %s K %d, %d stages, rate %g depth %d, at most %d nodes: restatement within %.1e / %.1e (row order %.1e / %.1e)"
          % ((what, X[tr].shape, K, stages, learning_rate, max_depth, counts.max()) + gaps))


def main():
    import sklearn
    from sklearn.ensemble import GradientBoostingClassifier
    store = {"kind": "boost_edges", "sklearn_version": sklearn.__version__, "stage0_names": np.array(list(E.STAGE0)),
             "whole_names": np.array(list(E.WHOLE)), "param_names": np.array(list(E.PARAMS)), "cut_rates": np.array(E.CUT_RATES)}

    for i, name in enumerate(E.STAGE0):
        X, y, K, rs = E.stage0_case(name)
        k_out = 1 if K == 2 else K
        m = B.sklearn_fit(X, y, 1, rs)
        seeds = B.tree_seeds(rs, k_out)
        live = [B.tree_arrays(m.estimators_[0, k].tree_) for k in range(k_out)]
        trees, score, raw, init = B.fit(X, y, K, 1, seeds)
        live_raw = m._raw_predict(X.astype(np.float32))
        for a, b in zip(trees, live):
            B.assert_same_tree(a, b, name)                             # the replayed stream, the structures AND the Newton values
        assert np.array_equal(init, m._raw_predict_init(X[:1].astype(np.float32))[0]) and np.array_equal(raw, live_raw), name
        assert rel(score, m.train_score_) <= GATE, name
        p = "s%d_" % i
        store.update({p + "digest": E.digest(X.astype(np.float32), y), p + "K": np.int64(K), p + "random_state": np.int64(rs),
                      p + "seeds": np.array(seeds), p + "init": init, p + "train_score": m.train_score_, p + "train_raw": live_raw})
        store_trees(store, p, live)
        print("%-28s %s K %d: %d trees, stage 0 equal, train_score_ within %.1e" % (name, X.shape, K, k_out, rel(score, m.train_score_)))

    for i, name in enumerate(E.WHOLE):
        whole_record(store, "w%d_" % i, name, E.whole_case(name), B.LEARNING_RATE, B.MAX_DEPTH)
    for i, (name, (rate, depth)) in enumerate(E.PARAMS.items()):
        whole_record(store, "p%d_" % i, name, E.param_case(), rate, depth)

    x32 = E.TWO_X.astype(np.float32)
    for i, rate in enumerate(E.CUT_RATES):
        m = GradientBoostingClassifier(n_estimators=1, learning_rate=rate, max_depth=1, init="zero", random_state=0).fit(x32, E.TWO_Y)
        raw = m._raw_predict(x32)
        assert np.array_equal(raw[:, 0], np.where(E.TWO_Y == 1, 2.0, -2.0) * rate), rate          # to the bit
        store.update({"l%d_train_score" % i: m.train_score_, "l%d_train_raw" % i: raw})
        print("rate %-6g raw %+.17g / %+.17g, train_score_ %.17g" % (rate, raw[0, 0], raw[-1, 0], m.train_score_[0]))

    for depth, nodes, last in ((20, 41, 2), (21, 43, 1)):               # (a peeled row goes right: the chain runs down the left, node d lies at depth d)
        c = E.chain_case(depth)
        tree = B.sklearn_tree(c["X"].astype(np.float32), c["y"], c["w"], B.FixedSeed(c["seed"]), depth)
        B.assert_same_tree(B.fit_tree(c["X"].astype(np.float32), c["y"], c["w"], c["seed"], depth), tree, "chain %d" % depth)
        leaves = tree["children_left"] < 0
        assert tree["feature"].shape[0] == nodes and leaves[depth] and not leaves[:depth].any() and tree["n_node_samples"][depth] == last, depth
        assert (tree["impurity"][depth] > 0.0) == (depth == 20) and (tree["impurity"][leaves] > 0.0).sum() == (depth == 20), depth
        p = "chain%d_" % depth
        store[p + "digest"] = E.digest(c["X"], c["y"], c["w"], c["mean"], c["scale"])
        for f in B.FIELDS:
            store[p + f] = tree[f]
        print("chain under max_depth %d: %d nodes, the deepest leaf holds %d rows, impurity %g" % (depth, nodes, last, tree["impurity"][depth]))

    np.savez_compressed(OUT, **store)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
