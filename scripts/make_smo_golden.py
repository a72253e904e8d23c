#!/usr/bin/env python3
"""Write tests/golden/smo_*.npz: the goldens of the batched SMO solver and the SVM split sweep (kernels_smo.hpp).

Runs scikit-learn on the host: SVC(C, kernel, probability=False, gamma='auto', tol=eps).fit on the standardised training rows of
a job, decision_function (libsvm's one-against-one values: decision_function_shape='ovo', and for two classes scikit-learn's
sign flip undone, so a positive value votes for the FIRST class) and predict on the job's test rows.  Every file has a `kind`
key and no object arrays.

  smo_binary (kind "smo_binary")   300 x 20 two-class data; cases c0_ .. over kernel x C x eps: train / test index lists, mean,
      scale, C, kernel type, eps, scikit-learn's decision values and labels, tol_dec
  smo_sweep_linear, smo_sweep_rbf (kind "smo_sweep")   240 x 20, 3 classes, 2 values of C x 3 splits as jobs in the form of
      paa_svc_fit_splits_f64; the training list of one split lacks a class (that job has one pair), one split has an empty test
      list; per job scikit-learn's decision values [Q][3] (zeros past the job's pairs), labels and tol_dec

tol_dec of a case: the measured distance |restatement - scikit-learn| / max|dec| (tests/smo_ref.py against scikit-learn; libsvm
keeps its kernel cache in float32, which moves the stopping point) times 4 -- a different rounding order of the kernel values
moves the stopping point again -- and at least 1e-9, the project's tight gate for kernel-value sums.
The label cap, asserted here on the reference alone: at most 2 % of a case's test rows have some pair with |dec| <= 2.5 tol_dec
max|dec| in scikit-learn's own values; only on those rows may a device label differ from scikit-learn's.

    python scripts/make_smo_golden.py            # needs scikit-learn
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smo_ref  # noqa: E402
import train_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def sklearn_job(X, y, job, kernel, eps):
    """(libsvm's decision values [n_test][pairs], predicted labels) of one job from scikit-learn."""
    import sklearn.svm
    tr, te, mean, scale, C = job
    clf = sklearn.svm.SVC(C=C, kernel=kernel, probability=False, gamma="auto", tol=eps, decision_function_shape="ovo")
    clf.fit((X[tr] - mean) / scale, y[tr])
    if len(te) == 0:
        k = len(clf.classes_)
        return np.zeros((0, k * (k - 1) // 2)), np.zeros(0)
    Zq = (X[te] - mean) / scale
    dec = clf.decision_function(Zq)
    dec = -dec.reshape(-1, 1) if len(clf.classes_) == 2 else dec
    return dec, clf.predict(Zq)


def measure(X, y, job, kernel, eps, what):
    """scikit-learn's answers of a job, the restatement's distance to them and the tolerance that follows; asserts the cap."""
    sk_dec, sk_pred = sklearn_job(X, y, job, kernel, eps)
    pred, dec, its, status, n_sv, classes = smo_ref.fit_job(X, y, job, kernel, None, eps)
    assert np.all(status == smo_ref.STATUS_CONVERGED)
    if sk_dec.shape[0] == 0:
        return sk_dec, sk_pred, 1e-9, 0.0
    scale = np.max(np.abs(sk_dec))
    dist = float(np.max(np.abs(dec - sk_dec)) / scale)
    tol = max(4.0 * dist, 1e-9)
    near = np.any(np.abs(sk_dec) <= 2.5 * tol * scale, axis=1)
    assert np.count_nonzero(near) <= 0.02 * sk_dec.shape[0], (what, int(np.count_nonzero(near)), sk_dec.shape[0])
    assert np.array_equal(pred[~near], sk_pred[~near]), what
    print("%-34s distance %.3g  tol_dec %.3g  near rows %d of %d  iterations %s" % (what, dist, tol, np.count_nonzero(near),
                                                                                     sk_dec.shape[0], its.tolist()))
    return sk_dec, sk_pred, tol, dist


def split_job(X, idx_train, idx_test, C):
    return (idx_train, idx_test, X[idx_train].mean(axis=0), X[idx_train].std(axis=0), C)


def make_binary():
    feats = train_ref.class_features((160, 140), 20, seed=21, spread=1.2)
    X, y = train_ref.features_to_matrix(feats)
    rng = np.random.default_rng(22)
    perm = rng.permutation(X.shape[0])
    tr, te = np.sort(perm[:200]), perm[200:]
    out = {"kind": np.array("smo_binary"), "X": X, "labels": y.astype(np.int32), "train_idx": tr.astype(np.int32),
           "test_idx": te.astype(np.int32)}
    cases = [(kernel, C, eps) for kernel in ("linear", "rbf") for C in (0.001, 1.0, 20.0) for eps in (1e-3,)]
    cases += [("linear", 1.0, 1e-9), ("rbf", 20.0, 1e-9)]
    for c, (kernel, C, eps) in enumerate(cases):
        job = split_job(X, tr, te, C)
        sk_dec, sk_pred, tol, dist = measure(X, y, job, kernel, eps, "binary %s C=%g eps=%g" % (kernel, C, eps))
        p = "c%d_" % c
        out.update({p + "kernel_type": np.array(smo_ref.KERNEL_TYPES[kernel]), p + "C": np.array(C), p + "eps": np.array(eps),
                    p + "mean": job[2], p + "scale": job[3], p + "sk_dec": sk_dec[:, 0], p + "sk_pred": sk_pred.astype(np.int32),
                    p + "tol_dec": np.array(tol), p + "distance": np.array(dist)})
    out["n_cases"] = np.array(len(cases))
    np.savez_compressed(os.path.join(OUT, "smo_binary.npz"), **out)


def make_sweep(kernel):
    feats = train_ref.class_features((100, 80, 60), 20, seed=31, spread=1.2)
    X, y = train_ref.features_to_matrix(feats)
    rng = np.random.default_rng(32)
    eps = 1e-3
    jobs = []
    for C in (0.5, 5.0):
        for s in range(3):
            perm = rng.permutation(X.shape[0])
            tr, te = perm[:200], perm[200:]
            if s == 1:
                tr = tr[y[tr] != 1]                     # the training list lacks class 1: one pair, (0, 2)
            if s == 2:
                te = te[:0]                             # an empty test list
            jobs.append(split_job(X, tr, te, C))
    out = {"kind": np.array("smo_sweep"), "X": X, "labels": y.astype(np.int32), "kernel_type": np.array(smo_ref.KERNEL_TYPES[kernel]),
           "eps": np.array(eps), "C": np.array([j[4] for j in jobs]), "mean": np.stack([j[2] for j in jobs]),
           "scale": np.stack([j[3] for j in jobs]),
           "train_off": np.concatenate([[0], np.cumsum([len(j[0]) for j in jobs])]).astype(np.int64),
           "test_off": np.concatenate([[0], np.cumsum([len(j[1]) for j in jobs])]).astype(np.int64),
           "train_idx": np.concatenate([j[0] for j in jobs]).astype(np.int32),
           "test_idx": np.concatenate([j[1] for j in jobs]).astype(np.int32)}
    decs, preds, tols, pairs = [], [], [], []
    for j, job in enumerate(jobs):
        sk_dec, sk_pred, tol, _ = measure(X, y, job, kernel, eps, "sweep %s job %d C=%g" % (kernel, j, job[4]))
        decs.append(np.pad(sk_dec, ((0, 0), (0, 3 - sk_dec.shape[1]))))
        preds.append(sk_pred)
        tols.append(tol)
        pairs.append(sk_dec.shape[1])
    out.update({"sk_dec": np.concatenate(decs), "sk_pred": np.concatenate(preds).astype(np.int32), "tol_dec": np.array(tols),
                "n_pairs": np.array(pairs, dtype=np.int32)})
    np.savez_compressed(os.path.join(OUT, "smo_sweep_%s.npz" % kernel), **out)


if __name__ == "__main__":
    make_binary()
    make_sweep("linear")
    make_sweep("rbf")
