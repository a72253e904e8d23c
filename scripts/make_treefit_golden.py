#!/usr/bin/env python3
"""Goldens of the GPU tree builder (audioTrainTest.tree_fit / forest_split_fit_predict / train_forest_device; kernels_treefit.hpp,
lib_treefit.hpp): scikit-learn's own trees and forests on the cases of tests/treefit_ref.py, recorded so that the tests can demand
EQUALITY -- integer arrays equal, float64 arrays bit-equal -- on a machine without scikit-learn, or with another version of it.

  tests/golden/treefit_edges.npz   treefit_ref.edge_cases(): per case c<i>_ the inputs X, y, w (integer weights), mean, scale and seed
                                   (the splitter's rand_r seed, handed to scikit-learn through a RandomState whose randint returns
                                   it), and per splitter ("best": DecisionTreeClassifier, "random": ExtraTreeClassifier, both
                                   max_features="sqrt") the tree_ arrays c<i>_<splitter>_<field> of treefit_ref.TREE_FIELDS and
                                   missing_go_to_left
  tests/golden/treefit_limit.npz   treefit_ref.limit_case(): 8192 rows, the row limit, both splitters
  tests/golden/treefit_wide.npz    treefit_ref.wide_limit_case(): 8192 rows, 64 classes, weights 0 / 1 / 3 / 8191, both splitters: the
                                   classifier's largest launch.  (The same rows with 32 classes would take the file past the
                                   largest golden in the tree; tests/test_treefit_scale_gpu.py walks that tree on the host instead)
  tests/golden/treefit_sweep.npz   treefit_ref.sweep_case(): X, y, per job j<i>_ train, test, mean, scale, n_estimators, seed, and per
                                   kind ("randomforest", "extratrees") predict and predict_proba of the test rows of
                                   <Kind>Classifier(n_estimators, random_state=seed) fitted on the standardised training rows;
                                   for job 2 also tree_states (estimators_[i].random_state) and in_bag (the bootstrap counts of
                                   every tree, from estimators_samples_)

Every file has kind "treefit", sklearn_version and names / n_jobs.  Before anything is written the NumPy restatement
(treefit_ref.fit_tree) is compared with every recorded tree: a difference stops the script.

    python scripts/make_treefit_golden.py            # needs scikit-learn (the goldens in the tree were made with 1.7.2)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import treefit_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FIELDS = R.TREE_FIELDS + ("missing_go_to_left",)


def record(store, prefix, case, check):
    k = int(np.unique(case["y"]).shape[0])
    x32 = R.standardize32(case["X"], case["mean"], case["scale"])
    for name in ("X", "y", "w", "mean", "scale"):
        store[prefix + name] = case[name]
    store[prefix + "seed"] = np.int64(case["seed"])
    trees = {}
    for sp in ("best", "random"):
        tree, seed = R.sklearn_tree(x32, case["y"], case["w"], k, R.FixedSeed(case["seed"]), sp)
        assert seed == case["seed"]
        if check:
            ours = R.fit_tree(x32, case["y"], case["w"], k, case["seed"], sp)
            for f in FIELDS:
                assert np.asarray(ours[f]).shape == tree[f].shape and np.array_equal(ours[f], tree[f]), (prefix, sp, f)
        for f in FIELDS:
            store["%s%s_%s" % (prefix, sp, f)] = tree[f]
        trees[sp] = tree
    return trees


def main():
    import sklearn
    head = {"kind": "treefit", "sklearn_version": sklearn.__version__}
    cases = R.edge_cases()
    store = dict(head, names=np.array(list(cases)))
    for i, (name, case) in enumerate(cases.items()):
        tree = record(store, "c%d_" % i, case, True)["random"]
        print("%-26s %5d rows %4d dims  random: %4d nodes" % (name, case["X"].shape[0], case["X"].shape[1], tree["feature"].shape[0]))
    np.savez_compressed(os.path.join(OUT, "treefit_edges.npz"), **store)

    store = dict(head, names=np.array(["row_limit"]))
    case = R.limit_case()
    case["X"] = case["X"].astype(np.float32)                  # every value is a float32: half the file
    tree = record(store, "c0_", case, False)["random"]
    print("row_limit: %d rows, random: %d nodes" % (case["X"].shape[0], tree["feature"].shape[0]))
    np.savez_compressed(os.path.join(OUT, "treefit_limit.npz"), **store)

    store = dict(head, names=np.array(["wide_limit_64"]))
    case = R.wide_limit_case()
    case["X"], case["y"] = case["X"].astype(np.float32), case["y"].astype(np.uint8)      # as small as the values allow
    trees = record(store, "c0_", case, False)
    print("wide_limit_64: %d rows, best: %d nodes, random: %d nodes" % (case["X"].shape[0], trees["best"]["feature"].shape[0],
                                                                        trees["random"]["feature"].shape[0]))
    np.savez_compressed(os.path.join(OUT, "treefit_wide.npz"), **store)
    assert os.path.getsize(os.path.join(OUT, "treefit_wide.npz")) <= os.path.getsize(os.path.join(OUT, "platt_dims.npz"))

    X, y, jobs = R.sweep_case()
    store = dict(head, X=X, y=y, n_jobs=np.int64(len(jobs)))
    for j, job in enumerate(jobs):
        for name, v in zip(("train", "test", "mean", "scale"), job[:4]):
            store["j%d_%s" % (j, name)] = v
        store["j%d_n_estimators" % j], store["j%d_seed" % j] = np.int64(job[4][0]), np.int64(job[4][1])
        for kind in ("randomforest", "extratrees"):
            label, proba, m = R.sklearn_forest(X, y, job, kind)
            store["j%d_%s_label" % (j, kind)], store["j%d_%s_proba" % (j, kind)] = label, proba
            if j == 2 and kind == "randomforest":
                store["j2_tree_states"] = np.array([e.random_state for e in m.estimators_], dtype=np.int64)
                store["j2_in_bag"] = np.stack([np.bincount(s, minlength=len(job[0])) for s in m.estimators_samples_]).astype(np.int32)
    np.savez_compressed(os.path.join(OUT, "treefit_sweep.npz"), **store)
    for f in ("treefit_edges.npz", "treefit_limit.npz", "treefit_wide.npz", "treefit_sweep.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
