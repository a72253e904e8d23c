#!/usr/bin/env python3
"""Write tests/golden/treefit_host_parent_bits.npz: every output of the tree fitters' host paths -- the boosting sweep
(paa_boost_fit_splits_f64), the forest sweeps (paa_forest_fit_splits_f64, paa_forest_reg_fit_splits_f64) and the builder entry points
(paa_tree_fit_tasks_f64, ..._reg_..., ..._boost_...) -- on small inputs, bit for bit, from the commit BEFORE the three fitters were put
on one host path (the job-class pass, TreeBatch for all three, one array read-back, one scorer; audioTrainTest.py's shared helpers).

The kernels are the same before and after and a tree is a function of its job alone, so a build that moves the host's offsets, chunk
tables, permutations and read-backs into shared pieces must reproduce every output exactly: a difference is an indexing mistake of
the host.  tests/test_treefit_host_bits_gpu.py runs the calls below on the build under test and asserts np.array_equal.

The inputs are seeded Gaussian features (no ties), N_SAMPLES x 5, the random-forest sweep at 34 dims.  check_coverage() states, from
the tables alone, what the calls reach: a caller's order of boosting jobs that is not the order of falling stage counts, a job whose
classes have gaps, empty test lists, two builder tasks that share a job, training lists of 256 and 257 rows and a bound on the
chunk bytes that cuts the boosting sweep into at least 3 chunks.  (All five stage counts of the boosting jobs differ, so every cut
falls where the bytes put it: between jobs 0 | 3 and 4 | 2 without the trees, 1 | 0 | 3 | 4 with them.)

    python scripts/make_treefit_host_bits_golden.py     # on the GPU, once, in a checkout of that earlier commit plus this file
"""
import argparse
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "treefit_host_parent_bits.npz")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_SAMPLES = 600
CLASS_COUNTS = (200, 200, 80, 40, 40, 40)         # samples per class 0 .. 5 of labels()
# the boosting sweep's jobs: (train rows, classes present, stages, test rows), in the caller's order
BOOST_JOBS = ((257, (0, 2, 5), 4, 0), (40, (1, 3), 6, 1), (256, (0, 1), 1, 65), (300, (0, 1, 2, 4), 3, 257), (2, (2, 3), 2, 64))
# the bound of the chunked runs and the chunks the earlier commit reports under it, by `trees` (41 more bytes per node with them)
BOOST_CHUNK_BYTES = 40000
BOOST_CHUNKS = {False: 3, True: 4}
# the regression sweep's jobs: (train rows, trees, test rows)
REG_JOBS = ((257, 3, 0), (1, 2, 1), (256, 1, 65), (33, 5, 257))
# the classifier sweeps' jobs: (train rows, classes present, trees, test rows)
FOREST_JOBS = ((257, (0, 1, 3), 3, 40), (64, (2, 5), 5, 0), (31, (0, 1, 2, 4, 5), 2, 65))
FOREST_DIMS = {"randomforest": 34, "extratrees": 5}
# the builder calls' tasks: (job, weights: None, "zero" (a row out of the bag), "bag" (bootstrap counts), "two" (every row twice));
# the tasks of a job pass the SAME rows / y / mean / scale objects
BUILDER_ROWS = (60, 33)
BUILDER_TASKS = ((0, None), (1, "zero"), (0, "bag"), (1, "two"))
BUILDERS = ("tree_fit_best", "tree_fit_random", "tree_fit_regression", "tree_fit_boosting")
BOOST_MODEL_FIELDS = ("node_offsets", "children_left", "children_right", "feature", "threshold", "missing_go_to_left", "value",
                      "classes_", "init", "impurity", "n_node_samples", "weighted_n_node_samples", "class_prior_", "train_score_")
TREE_FIELDS = ("children_left", "children_right", "feature", "threshold", "impurity", "n_node_samples", "weighted_n_node_samples",
               "missing_go_to_left", "value")


@functools.lru_cache(maxsize=None)
def matrix(n_dims):
    """(X [N_SAMPLES][n_dims], labels, targets): Gaussian features, shuffled class indices with CLASS_COUNTS, Gaussian targets.
    Read-only."""
    rng = np.random.default_rng(2000 + n_dims)
    X = rng.standard_normal((N_SAMPLES, n_dims)) * rng.uniform(0.5, 2.0, n_dims) + rng.normal(0, 2, n_dims)
    labels = rng.permutation(np.repeat(np.arange(len(CLASS_COUNTS)), CLASS_COUNTS)).astype(np.int64)
    targets = X @ (rng.standard_normal(n_dims) / np.sqrt(n_dims)) + rng.standard_normal(N_SAMPLES)
    for a in (X, labels, targets):
        a.setflags(write=False)
    return X, labels, targets


def _split(rng, X, labels, n, classes, n_test, last):
    """A job (train, test, mean, scale, last): n training rows that hold exactly `classes` (None: any rows), n_test test rows."""
    if classes is None:
        train = rng.permutation(N_SAMPLES)[:n]
    else:
        first = [rng.choice(np.flatnonzero(labels == c)) for c in classes]
        rest = np.setdiff1d(np.flatnonzero(np.isin(labels, classes)), first)
        train = rng.permutation(np.concatenate([first, rng.permutation(rest)[:n - len(first)]]))
        assert train.shape[0] == n and set(labels[train]) == set(classes)
    src = X[train] if n > 3 else X                  # a scale of 0 would flag the job
    return train, rng.permutation(N_SAMPLES)[:n_test], src.mean(axis=0), src.std(axis=0), last


def boost_jobs():
    X, labels, _ = matrix(5)
    rng = np.random.default_rng(31)
    return [_split(rng, X, labels, n, classes, n_test, (stages, 100 + j)) for j, (n, classes, stages, n_test) in enumerate(BOOST_JOBS)]


def reg_jobs():
    X, labels, _ = matrix(5)
    rng = np.random.default_rng(32)
    return [_split(rng, X, labels, n, None, n_test, (trees, 200 + j)) for j, (n, trees, n_test) in enumerate(REG_JOBS)]


def forest_jobs(kind):
    X, labels, _ = matrix(FOREST_DIMS[kind])
    rng = np.random.default_rng(33)
    return [_split(rng, X, labels, n, classes, n_test, (trees, 300 + j)) for j, (n, classes, trees, n_test) in enumerate(FOREST_JOBS)]


def builder_tasks(regression):
    X, labels, targets = matrix(5)
    rng = np.random.default_rng(34)
    jobs = []
    for n in BUILDER_ROWS:
        rows = rng.permutation(N_SAMPLES)[:n]
        jobs.append((rows, (targets if regression else labels)[rows], X[rows].mean(axis=0), X[rows].std(axis=0)))
    tasks = []
    for t, (j, how) in enumerate(BUILDER_TASKS):
        rows, y, mean, scale = jobs[j]
        n = rows.shape[0]
        w = {None: None, "zero": np.where(np.arange(n) == 1, 0, 1), "bag": np.bincount(rng.integers(0, n, n), minlength=n),
             "two": np.full(n, 2)}[how]
        tasks.append((rows, y, w, 1000 + 17 * t, mean, scale))
    return tasks


def call_names():
    """Every call of the record, in order."""
    names = ["boost_trees%d_%s" % (trees, chunk) for trees in (1, 0) for chunk in ("default", "chunked")]
    names += ["reg_train_pred%d" % tp for tp in (1, 0)]
    names += ["forest_%s" % kind for kind in FOREST_DIMS]
    return names + list(BUILDERS)


def expected_keys(name):
    """The outputs of a call, from the tables."""
    if name.startswith("boost_"):
        keys = ["label", "proba", "n_chunks"]
        if name.startswith("boost_trees1"):
            for j in range(len(BOOST_JOBS)):
                keys += ["train_score.%d" % j, "train_raw.%d" % j, "train_resid.%d" % j]
                keys += ["models.%d.%s" % (j, f) for f in BOOST_MODEL_FIELDS]
        return keys
    if name.startswith("reg_"):
        return ["pred", "n_chunks"] + (["train_pred"] if name.endswith("1") else [])
    if name.startswith("forest_"):
        return ["label", "proba", "n_chunks"]
    keys = ["trees.%d.%s" % (t, f) for t in range(len(BUILDER_TASKS)) for f in TREE_FIELDS]
    return keys + (["classes.%d" % t for t in range(len(BUILDER_TASKS))] if name in BUILDERS[:2] else [])


def run(name):
    """{output: array} of one call on the library in use."""
    from pyaudioanalysis_amd import audioTrainTest as aT
    out = {}
    if name.startswith("boost_"):
        trees = name.startswith("boost_trees1")
        X, labels, _ = matrix(5)
        res = aT.boosting_split_fit_predict(X, labels, boost_jobs(), proba=True, train_score=trees, trees=trees,
                                            chunk_bytes=BOOST_CHUNK_BYTES if name.endswith("chunked") else None)
        out.update(label=res.label, proba=res.proba, n_chunks=np.array(res.n_chunks))
        for j in range(len(BOOST_JOBS) if trees else 0):
            out["train_score.%d" % j], out["train_raw.%d" % j], out["train_resid.%d" % j] = res.train_score[j], res.train_raw[j], res.train_resid[j]
            for f in BOOST_MODEL_FIELDS:
                out["models.%d.%s" % (j, f)] = np.asarray(getattr(res.models[j], f))
    elif name.startswith("reg_"):
        X, _, targets = matrix(5)
        res = aT.forest_regression_split_fit_predict(X, targets, reg_jobs(), train_pred=name.endswith("1"))
        out.update(pred=res.pred, n_chunks=np.array(res.n_chunks))
        if res.train_pred is not None:
            out["train_pred"] = res.train_pred
    elif name.startswith("forest_"):
        kind = name[len("forest_"):]
        X, labels, _ = matrix(FOREST_DIMS[kind])
        res = aT.forest_split_fit_predict(X, labels, forest_jobs(kind), kind, proba=True)
        out.update(label=res.label, proba=res.proba, n_chunks=np.array(res.n_chunks))
    else:
        X = matrix(5)[0]
        if name == "tree_fit_regression":
            res = aT.tree_fit_regression(X, builder_tasks(True))
        elif name == "tree_fit_boosting":
            res = aT.tree_fit_boosting(X, builder_tasks(True), max_depth=2)
        else:
            res = aT.tree_fit(X, builder_tasks(False), name[len("tree_fit_"):])
        for t, tree in enumerate(res.trees):
            for f in TREE_FIELDS:
                out["trees.%d.%s" % (t, f)] = tree[f]
            if res.classes is not None:
                out["classes.%d" % t] = np.asarray(res.classes[t])
    return {k: np.asarray(v) for k, v in out.items()}


def check_coverage():
    """What the record was asked to reach, from the tables alone."""
    stages = [s for _, _, s, _ in BOOST_JOBS]
    assert sorted(range(len(stages)), key=lambda j: -stages[j]) != list(range(len(stages))), "the caller's order is the stage order"
    assert len(set(stages)) == len(stages) == 5
    for jobs in (BOOST_JOBS, FOREST_JOBS):
        assert any(list(c) != list(range(len(c))) and max(c) - min(c) + 1 > len(c) for _, c, _, _ in jobs), "no job with a class gap"
        assert any(job[-1] == 0 for job in jobs), "no empty test list"
        assert len({len(c) for _, c, _, _ in jobs}) > 1
    assert any(len(c) == 2 for _, c, _, _ in BOOST_JOBS) and any(len(c) > 2 for _, c, _, _ in BOOST_JOBS)       # one output and several
    assert any(job[-1] == 0 for job in REG_JOBS) and any(job[0] == 1 for job in REG_JOBS)
    assert len({job[2] for job in FOREST_JOBS}) == len(FOREST_JOBS) and len({job[1] for job in REG_JOBS}) == len(REG_JOBS)
    for jobs in (BOOST_JOBS, REG_JOBS, FOREST_JOBS):
        assert {job[0] for job in jobs} & {255, 256, 257}, "no training list at 255 .. 257 rows"
        assert any(job[-1] > 256 for job in jobs) or jobs is FOREST_JOBS
    task_jobs = [j for j, _ in BUILDER_TASKS]
    assert len(task_jobs) == 4 and len(set(task_jobs)) == 2 and any(task_jobs.count(j) > 1 for j in task_jobs), "no two tasks share a job"
    assert {how for _, how in BUILDER_TASKS} >= {None, "zero"}
    assert all(v >= 3 for v in BOOST_CHUNKS.values()) and BOOST_CHUNKS[True] != BOOST_CHUNKS[False]
    assert set(FOREST_DIMS) == {"randomforest", "extratrees"} and 34 in FOREST_DIMS.values()
    for n, classes, _, _ in BOOST_JOBS + FOREST_JOBS:
        assert sum(CLASS_COUNTS[c] for c in classes) >= n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--check", action="store_true", help="assert the coverage of the tables on the CPU and stop")
    args = ap.parse_args()
    check_coverage()
    if args.check:
        print("coverage ok")
        return
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import device_code_hash
    arrays = {}
    for name in call_names():
        got = run(name)
        assert set(got) == set(expected_keys(name)), (name, sorted(set(got) ^ set(expected_keys(name))))
        if name.startswith("boost_"):
            want = BOOST_CHUNKS[name.startswith("boost_trees1")] if name.endswith("chunked") else 1
            assert int(got["n_chunks"]) == want, (name, int(got["n_chunks"]), want)
        for key, value in got.items():
            arrays["%s.%s" % (name, key)] = value
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, kind=np.array("treefit_host_bits"), compiler=np.array(device_code_hash.compiler_id() or ""), **arrays)
    print("%s: %d outputs, %d bytes" % (args.out, len(arrays), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
