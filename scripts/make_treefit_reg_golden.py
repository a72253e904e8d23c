#!/usr/bin/env python3
"""Goldens of the GPU regression-tree builder (audioTrainTest.tree_fit_regression / forest_regression_split_fit_predict /
train_random_forest_regression_device; kernels_treefit.hpp K19, lib_treefit.hpp): scikit-learn's own regression trees and forests on
the cases of tests/treefit_reg_ref.py, recorded so that the tests can demand EQUALITY -- integer arrays equal, float64 arrays
bit-equal -- on a machine without scikit-learn, or with another version of it.  Equality can be demanded because every case keeps
the exactness premise, which this script asserts before it records anything: all targets are multiples of 1/8 within +-1024 and
every tree's total weight is at most 8192, so every sum of the criterion is exact in FP64 and its order is immaterial.

  tests/golden/treefit_reg_edges.npz   treefit_reg_ref.edge_cases(): per case c<i>_ the inputs X, y, w (integer weights), mean, scale
                                       and seed (the splitter's rand_r seed, handed to scikit-learn through a RandomState whose
                                       randint returns it) and the tree_ arrays c<i>_<field> of DecisionTreeRegressor()
  tests/golden/treefit_reg_limit.npz   treefit_reg_ref.limit_case(): 8192 in-bag rows, the row limit
  tests/golden/treefit_reg_sweep.npz   treefit_reg_ref.sweep_case(): X, y, per job j<i>_ train, test, mean, scale, n_estimators, seed
                                       and predict of the test rows (j<i>_pred) and of the training rows (j<i>_train_pred) of
                                       RandomForestRegressor(n_estimators, random_state=seed) fitted on the standardised training rows

Every file has kind "treefit_reg", sklearn_version and names / n_jobs.  Before anything is written the NumPy restatement
(treefit_reg_ref.fit_tree) is compared with every recorded tree: a difference stops the script.

    python scripts/make_treefit_reg_golden.py        # needs scikit-learn (the goldens in the tree were made with 1.7.2)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import treefit_reg_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def record(store, prefix, case):
    R.assert_exact(case["y"], case["w"])
    x32 = R.standardize32(case["X"], case["mean"], case["scale"])
    for name in ("X", "y", "w", "mean", "scale"):
        store[prefix + name] = case[name]
    store[prefix + "seed"] = np.int64(case["seed"])
    tree = R.sklearn_tree(x32, case["y"], case["w"], R.FixedSeed(case["seed"]))
    ours = R.fit_tree(x32, case["y"], case["w"], case["seed"])
    for f in R.FIELDS:
        assert np.asarray(ours[f]).shape == tree[f].shape and np.array_equal(ours[f], tree[f]), (prefix, f)
        store[prefix + f] = tree[f]
    return tree


def main():
    import sklearn
    head = {"kind": "treefit_reg", "sklearn_version": sklearn.__version__}
    cases = R.edge_cases()
    store = dict(head, names=np.array(list(cases)))
    for i, (name, case) in enumerate(cases.items()):
        tree = record(store, "c%d_" % i, case)
        print("%-28s %5d rows %4d dims %5d nodes" % (name, case["X"].shape[0], case["X"].shape[1], tree["feature"].shape[0]))
    np.savez_compressed(os.path.join(OUT, "treefit_reg_edges.npz"), **store)

    store = dict(head, names=np.array(["row_limit"]))
    case = R.limit_case()
    case["X"] = case["X"].astype(np.float32)                  # every value is a float32: half the file
    tree = record(store, "c0_", case)
    print("row_limit: %d rows, %d nodes" % (case["X"].shape[0], tree["feature"].shape[0]))
    np.savez_compressed(os.path.join(OUT, "treefit_reg_limit.npz"), **store)

    X, y, jobs = R.sweep_case()
    store = dict(head, X=X, y=y, n_jobs=np.int64(len(jobs)))
    for j, job in enumerate(jobs):
        R.assert_exact(y[job[0]], np.ones(len(job[0]), dtype=np.int64))          # a bootstrap keeps the total weight
        for name, v in zip(("train", "test", "mean", "scale"), job[:4]):
            store["j%d_%s" % (j, name)] = v
        store["j%d_n_estimators" % j], store["j%d_seed" % j] = np.int64(job[4][0]), np.int64(job[4][1])
        store["j%d_pred" % j], store["j%d_train_pred" % j], _ = R.sklearn_forest(X, y, job)
    np.savez_compressed(os.path.join(OUT, "treefit_reg_sweep.npz"), **store)
    for f in ("treefit_reg_edges.npz", "treefit_reg_limit.npz", "treefit_reg_sweep.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
