#!/usr/bin/env python3
"""Goldens of the GPU gradient-boosting fit (audioTrainTest.tree_fit_boosting / boosting_split_fit_predict /
train_gradient_boosting_device; kernels_boost.hpp, kernels_treefit.hpp K20, lib_boost.hpp), from LIVE scikit-learn on the cases of
tests/boost_ref.py:

  tests/golden/boost_builder.npz   boost_ref.builder_cases() and limit_case(): per case c<i>_ the tree_ arrays of
                                   DecisionTreeRegressor(criterion="friedman_mse", max_depth, random_state -> the case's rand_r seed).
                                   Targets are multiples of 1/8 within +-1024 (asserted): the tests demand equality.  The inputs are
                                   not stored: boost_ref regenerates them (the file carries a checksum of each)
  tests/golden/boost_stage0.npz    boost_ref.STAGE0: balanced jobs of 2, 4 and 8 classes, GradientBoostingClassifier(n_estimators=1,
                                   random_state): X, y, the trees' rand_r seeds (the replayed RandomState stream), init, every tree's
                                   arrays WITH its Newton leaf values, train_score_ and the training raw predictions.  Stage 0 of a
                                   balanced job is exact: the tests demand equality
  tests/golden/boost_whole.npz     boost_ref.WHOLE: whole fits (10, 10 and 5 stages): X, y, train / held-out rows, seeds, init,
                                   train_score_, the training raw predictions and predict_proba of the held-out rows

Before anything is written the NumPy restatement (boost_ref.fit, which sums in the device's order) is compared with every record:
equality where the sums are exact, else train_score_ and raw predictions within 1e-9 relative -- and within the same gate when the
restatement sums in plain row order instead, so that no frozen case sits where two summation orders part (such a seed is to be
replaced).

    python scripts/make_boost_golden.py        # needs scikit-learn (the goldens in the tree were made with 1.7.2)
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import boost_ref as B  # noqa: E402
import treefit_reg_ref as RR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
GATE = 1e-9


def digest(case):
    h = hashlib.sha256()
    for name in ("X", "y", "w", "mean", "scale"):
        h.update(np.ascontiguousarray(case[name]).tobytes())
    return h.hexdigest()


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), np.finfo(np.float64).tiny))) if a.size else 0.0


def store_trees(store, prefix, trees):
    store[prefix + "node_offsets"] = np.concatenate([[0], np.cumsum([t["feature"].shape[0] for t in trees])]).astype(np.int64)
    for f in B.FIELDS:
        store[prefix + f] = np.concatenate([np.asarray(t[f]).reshape(-1) for t in trees])


def main():
    import sklearn
    head = {"kind": "boost", "sklearn_version": sklearn.__version__}

    cases = dict(B.builder_cases(), row_limit=B.limit_case())
    store = dict(head, names=np.array(list(cases)))
    for i, (name, c) in enumerate(cases.items()):
        RR.assert_exact(c["y"], c["w"])
        x32 = B.standardize32(c["X"], c["mean"], c["scale"])
        tree = B.sklearn_tree(x32, c["y"], c["w"], B.FixedSeed(c["seed"]), c["max_depth"])
        B.assert_same_tree(B.fit_tree(x32, c["y"], c["w"], c["seed"], c["max_depth"]), tree, name)
        store["c%d_digest" % i] = digest(c)
        for f in B.FIELDS:
            store["c%d_%s" % (i, f)] = tree[f]
        print("%-28s %5d rows %4d dims depth %2d %5d nodes" % (name, c["X"].shape[0], c["X"].shape[1], c["max_depth"], tree["feature"].shape[0]))
    np.savez_compressed(os.path.join(OUT, "boost_builder.npz"), **store)

    store = dict(head, names=np.array(list(B.STAGE0)))
    for i, name in enumerate(B.STAGE0):
        X, y, K, rs = B.stage0_case(name)
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
        store.update({p + "X": X.astype(np.float32), p + "y": y, p + "K": np.int64(K), p + "random_state": np.int64(rs), p + "seeds": np.array(seeds),
                      p + "init": init, p + "train_score": m.train_score_, p + "train_raw": live_raw})
        store_trees(store, p, live)
        print("%-28s %s K %d: %d trees, stage 0 equal" % (name, X.shape, K, k_out))
    np.savez_compressed(os.path.join(OUT, "boost_stage0.npz"), **store)

    store = dict(head, names=np.array(list(B.WHOLE)))
    for i, name in enumerate(B.WHOLE):
        X, y, tr, te, K, stages, rs = B.whole_case(name)
        k_out = 1 if K == 2 else K
        m = B.sklearn_fit(X[tr], y[tr], stages, rs)
        seeds = B.tree_seeds(rs, stages * k_out)
        live_raw = m._raw_predict(X[tr].astype(np.float32))
        trees, score, raw, init = B.fit(X[tr], y[tr], K, stages, seeds)
        keep = B.dev_sum, B.dev_prefix                                 # the other order: plain row order
        B.dev_sum = lambda v: np.float64(np.cumsum(v)[-1]) if len(v) else np.float64(0.0)
        B.dev_prefix = lambda v: np.concatenate([[0.0], np.cumsum(v)[:-1]])
        _, score2, raw2, _ = B.fit(X[tr], y[tr], K, stages, seeds)
        B.dev_sum, B.dev_prefix = keep
        gaps = (rel(score, m.train_score_), rel(raw, live_raw), rel(score2, m.train_score_), rel(raw2, live_raw))
        assert max(gaps) <= GATE, (name, gaps, "two summation orders part beyond the gate: replace this case's seed")
        p = "w%d_" % i
        store.update({p + "X": X.astype(np.float32), p + "y": y, p + "train": tr, p + "test": te, p + "K": np.int64(K), p + "n_stages": np.int64(stages),
                      p + "random_state": np.int64(rs), p + "seeds": np.array(seeds), p + "init": init, p + "train_score": m.train_score_,
                      p + "train_raw": live_raw, p + "test_proba": m.predict_proba(X[te].astype(np.float32))})
        print("%-28s %s K %d, %d stages: restatement within %.1e / %.1e (row order %.1e / %.1e)" % ((name, X[tr].shape, K, stages) + gaps))
    np.savez_compressed(os.path.join(OUT, "boost_whole.npz"), **store)


if __name__ == "__main__":
    main()
