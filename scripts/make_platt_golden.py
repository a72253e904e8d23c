#!/usr/bin/env python3
"""Goldens of the probabilistic SVM fit (audioTrainTest.svc_fit_proba / train_svm_device; kernels_platt.hpp, lib_smo.hpp):
scikit-learn's SVC(probability=True, random_state=r) on small synthetic cases, and the measured distance of the FP64 CPU
restatement (tests/platt_ref.py over tests/smo_ref.py) to it, which sets the tolerance the device results are held to.

  tests/golden/platt_small.npz   the cases of tests/test_platt_cpu.py, linear and RBF: two classes (30 / 25 rows), three classes of
                                 25 / 14 / 3 rows, 13 / 2 rows under a random_state whose folds include degenerate ones (a
                                 training part without the small class), and l = 4 (2 / 2 rows: an empty fold)
  tests/golden/platt_dims.npz    two classes at n_dims 1, 8, 9, 68, 136 and 256, linear and RBF
  tests/golden/platt_big.npz     a pair of 150 + 163 rows (more than one scoring tile of 16 rows and than the 32 rows a workgroup
                                 takes per step), linear and RBF, and two jobs that differ in rows, C and random_state

Every file has kind "platt" and n_cases.  Per case c<i>_: X, labels, train_idx, test_idx (held-back rows), mean, scale (of the training rows), C, kernel_type, random_state,
seed (libsvm's random_seed: np.random.RandomState(random_state).randint(np.iinfo('i').max)); scikit-learn's probA_, probB_,
_dual_coef_ scattered to the training rows (coef [k - 1][n_train]), _intercept_ and predict_proba of the held-back rows; sk_cv_dec,
the held-out decision values of scikit-learn's own probability=False fits on the restatement's folds, in pair-row order, pair
after pair, and `degenerate`, the rows whose value is a constant.  With those fold fits the restatement's sigmoid reproduces
probA_ / probB_ within 1e-9, asserted here: the folds are libsvm's.

Tolerances, as scripts/make_smo_golden.py measures tol_dec: per case the distance |restatement - scikit-learn| of each quantity --
ab: probA_ / probB_ over max(1, |A|, |B|); cv: the held-out values over max |value|; proba: the probabilities, absolute -- stored
as dist_<q>, and tol_<q> = 4 dist_<q>, at least 1e-9.  libsvm stops at eps = 1e-3 and keeps a float32 kernel cache, so the
distance is the stopping tolerance; a different rounding order of the kernel values moves the stopping point again, hence the factor 4, that script's margin.  No label is
compared, so there is no "near a decision" exclusion.  The coefficients and intercepts are stored for inspection and carry no
tolerance: inside the stopping tolerance the dual solution is far less determined than the decision values it produces (a row
may enter or leave the support set), so a restatement that happens to land on scikit-learn's coefficients says nothing about
the next rounding order; the printed coef distance is for the reader.  What holds the coefficients is predict_proba of the
held-back rows.

    python scripts/make_platt_golden.py            # needs scikit-learn
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import platt_ref  # noqa: E402
import smo_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
N_TEST = 12


def data(sizes, n_dims, seed):
    """(X, labels, train_idx, test_idx): Gaussian classes 1.6 / sqrt(n_dims) apart per dim, rows shuffled, N_TEST rows held back."""
    rng = np.random.RandomState(seed)
    sizes = list(sizes)
    k = len(sizes)
    lab = np.concatenate([np.full(n, c) for c, n in enumerate(sizes)] + [np.arange(N_TEST) % k]).astype(np.int32)
    X = rng.randn(lab.shape[0], n_dims) * rng.uniform(0.5, 2.0, n_dims) + rng.normal(0, 2, n_dims)
    X += 1.6 * lab[:, None] / np.sqrt(n_dims)
    n_train = sum(sizes)
    return X, lab, rng.permutation(n_train).astype(np.int32), np.arange(n_train, lab.shape[0], dtype=np.int32)


def degenerate_state(sizes, first=0):
    """The first random_state >= first whose folds of a two-class pair of `sizes` rows include a degenerate one."""
    signs = np.concatenate([np.ones(sizes[0]), -np.ones(sizes[1])])
    for r in range(first, first + 1000):
        seed = np.random.RandomState(r).randint(np.iinfo('i').max)
        if any(train is None and len(held) for held, train, _ in platt_ref.pair_folds(signs, seed)):
            return r
    raise AssertionError("no degenerate fold found")


def measure(name, X, lab, train_idx, test_idx, C, kernel, random_state):
    import sklearn.svm
    from pyaudioanalysis_amd import audioTrainTest as aT
    n_dims = X.shape[1]
    mean, scale = X[train_idx].mean(axis=0), X[train_idx].std(axis=0)
    scale = np.where(scale > 0, scale, 1.0)
    Z, Zq = (X[train_idx] - mean) / scale, (X[test_idx] - mean) / scale
    sk = sklearn.svm.SVC(C=C, kernel=kernel, probability=True, gamma="auto", random_state=random_state).fit(Z, lab[train_idx])
    seed = int(np.random.RandomState(random_state).randint(np.iinfo('i').max))
    job = (train_idx, mean, scale, C)

    def fold_dec(Zt, y, C_, Zh):
        m = sklearn.svm.SVC(C=C_, kernel=kernel, gamma=1.0 / n_dims).fit(Zt, y)
        return m.decision_function(Zh) * (1.0 if m.classes_[1] == 1 else -1.0)

    # the folds are libsvm's: scikit-learn's own fold fits reproduce probA_ / probB_
    _, sk_pairs = platt_ref.fit(X, lab, job, seed, kernel, fold_dec=fold_dec)
    ab = np.array([[q["prob_a"], q["prob_b"]] for q in sk_pairs])
    assert np.max(np.abs(ab - np.stack([sk.probA_, sk.probB_], axis=1))) <= 1e-9, name
    # the restatement
    classes, pairs = platt_ref.fit(X, lab, job, seed, kernel)
    assert all(np.all(q["status"][q["status"] != 0] == smo_ref.STATUS_CONVERGED) for q in pairs), name
    assert all(q["sigmoid_stop"] == platt_ref.STOP_CONVERGED for q in pairs), name
    model = platt_ref.model_of(X, lab, job, classes, pairs, kernel)
    k = len(classes)
    sk_coef, coef = np.zeros((k - 1, len(train_idx))), np.zeros((k - 1, len(train_idx)))
    sk_coef[:, sk.support_] = sk._dual_coef_
    coef[:, model.support_] = model._dual_coef_
    ref_ab = np.array([[q["prob_a"], q["prob_b"]] for q in pairs])
    sk_cv, cv = np.concatenate([q["cv_dec"] for q in sk_pairs]), np.concatenate([q["cv_dec"] for q in pairs])
    degenerate = np.concatenate([q["degenerate"] for q in pairs])
    sk_proba, proba = sk.predict_proba(Zq), aT.to_sklearn_svc(model).predict_proba(Zq)
    dist = {"ab": float(np.max(np.abs(ref_ab - ab) / np.maximum(1.0, np.max(np.abs(ab), axis=1, keepdims=True)))),
            "cv": float(np.max(np.abs(cv - sk_cv)) / np.max(np.abs(sk_cv))),
            "proba": float(np.max(np.abs(proba - sk_proba)))}
    coef_dist = max(np.max(np.abs(coef - sk_coef)) / C,
                    np.max(np.abs(model._intercept_ - sk._intercept_) / np.maximum(1.0, np.abs(sk._intercept_))))
    assert np.array_equal(cv[degenerate], sk_cv[degenerate])
    print("%-22s %-6s l %s  degenerate rows %d  distances %s (coef %.3g)  sigmoid margins %s" % (
        name, kernel, [len(q["rows"]) for q in pairs], np.count_nonzero(degenerate),
        " ".join("%s %.3g" % kv for kv in dist.items()), coef_dist, ["%.2g" % q["sigmoid_margin"] for q in pairs]))
    out = {"name": np.array(name), "X": X, "labels": lab, "train_idx": train_idx, "test_idx": test_idx, "mean": mean, "scale": scale,
           "C": np.array(float(C)), "kernel_type": np.array(smo_ref.KERNEL_TYPES[kernel]), "random_state": np.array(random_state),
           "seed": np.array(seed), "sk_probA": sk.probA_, "sk_probB": sk.probB_, "sk_coef": sk_coef, "sk_intercept": sk._intercept_,
           "sk_proba": sk_proba, "sk_cv_dec": sk_cv, "degenerate": degenerate}
    for q, d in dist.items():
        out["dist_" + q] = np.array(d)
        out["tol_" + q] = np.array(max(4.0 * d, 1e-9))
    return out


def write(file_name, cases):
    out = {"kind": np.array("platt"), "n_cases": np.array(len(cases))}
    for i, case in enumerate(cases):
        out.update({"c%d_%s" % (i, k): v for k, v in case.items()})
    path = os.path.join(OUT, file_name)
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


def main():
    small, dims, big = [], [], []
    for kernel in ("linear", "rbf"):
        small.append(measure("two_classes", *data((30, 25), 6, 11), 1.0, kernel, 3))
        small.append(measure("three_classes", *data((25, 14, 3), 6, 12), 1.0, kernel, 7))
        small.append(measure("degenerate_13_2", *data((13, 2), 4, 13), 1.0, kernel, degenerate_state((13, 2))))
        small.append(measure("l4", *data((2, 2), 3, 14), 1.0, kernel, 5))
        for d in (1, 8, 9, 68, 136, 256):
            dims.append(measure("dims_%d" % d, *data((24, 20), d, 20 + d), 1.0, kernel, d))
        big.append(measure("big_pair", *data((150, 163), 8, 31), 1.0, kernel, 9))
    X, lab, tr, te = data((40, 36, 30), 9, 32)
    big.append(measure("two_jobs_0", X, lab, np.sort(tr)[::2].copy(), te, 0.5, "linear", 21))
    big.append(measure("two_jobs_1", X, lab, tr[tr % 3 != 0].copy(), te, 5.0, "linear", 22))
    write("platt_small.npz", small)
    write("platt_dims.npz", dims)
    write("platt_big.npz", big)


if __name__ == "__main__":
    main()
