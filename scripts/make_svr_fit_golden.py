#!/usr/bin/env python3
"""Write tests/golden/svr_fit_*.npz: the goldens of the batched epsilon-SVR solver and the SVR split sweep (kernels_svrfit.hpp).

Runs scikit-learn on the host: SVR(C, kernel, epsilon=0.1, tol=eps).fit on the standardised training rows of a job (gamma stays
at SVR's default, 'scale') and predict on the job's test rows.  Every file has a `kind` key and no object arrays.

  svr_fit_linear, svr_fit_rbf (kind "svr_fit")   240 x 12 samples, a smooth target plus noise; 3 values of C x 2 splits as jobs in
      the form of paa_svr_fit_splits_f64 with test lists of 0, 1, 31, 32, 33 and 97 rows; per job scikit-learn's predictions,
      its support-vector count and tol_pred

tol_pred of a job: the measured distance |restatement - scikit-learn| / max|pred| (tests/svr_fit_ref.py against scikit-learn;
libsvm keeps its kernel cache in float32, which moves the stopping point) times 4 -- a different rounding order of the kernel
values moves the stopping point again -- and at least 1e-9, the project's tight gate for kernel-value sums.  Measured against
scikit-learn, never against the device.

    python scripts/make_svr_fit_golden.py            # needs scikit-learn
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smo_ref  # noqa: E402
import svr_fit_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TEST_LENGTHS = (0, 1, 31, 32, 33, 97)
N_TRAIN = 140


def regression_data(n, n_dims, seed):
    """(X [n][n_dims] on features of unequal scale and offset, y [n]: a smooth function of three directions plus noise)."""
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((n, n_dims))
    w = rng.standard_normal((3, n_dims)) / np.sqrt(n_dims)
    y = 2.0 + np.tanh(U @ w[0]) + 0.5 * (U @ w[1]) + 0.3 * np.sin(2.0 * (U @ w[2])) + 0.1 * rng.standard_normal(n)
    return U * rng.uniform(0.5, 3.0, n_dims) + rng.uniform(-2.0, 2.0, n_dims), y


def sklearn_job(X, y, job, kernel, eps):
    """(predictions of the test rows, number of support vectors) of one job from scikit-learn."""
    import sklearn.svm
    tr, te, mean, scale, C = job
    svr = sklearn.svm.SVR(C=C, kernel=kernel, epsilon=svr_fit_ref.SVR_EPSILON, tol=eps)
    svr.fit((X[tr] - mean) / scale, y[tr])
    return (svr.predict((X[te] - mean) / scale) if len(te) else np.zeros(0)), int(svr.support_.shape[0])


def measure(X, y, job, kernel, eps, what):
    """scikit-learn's answers of a job, the restatement's distance to them and the tolerance that follows."""
    sk_pred, sk_n_sv = sklearn_job(X, y, job, kernel, eps)
    pred, _, _, _, it, status, n_sv, _ = svr_fit_ref.fit_job(X, y, job, kernel, None, svr_fit_ref.SVR_EPSILON, eps)
    assert status == smo_ref.STATUS_CONVERGED
    dist = float(np.max(np.abs(pred - sk_pred)) / np.max(np.abs(sk_pred))) if len(sk_pred) else 0.0
    tol = max(4.0 * dist, 1e-9)
    print("%-30s distance %.3g  tol_pred %.3g  n_sv %d (scikit-learn %d)  iterations %d" % (what, dist, tol, n_sv, sk_n_sv, it))
    return sk_pred, sk_n_sv, tol, dist


def make(kernel):
    X, y = regression_data(240, 12, seed=51)
    rng = np.random.default_rng(52)
    eps = 1e-3
    jobs = []
    for C in (0.01, 0.1, 1.0):
        for _ in range(2):
            perm = rng.permutation(X.shape[0])
            tr, te = perm[:N_TRAIN], perm[N_TRAIN:N_TRAIN + TEST_LENGTHS[len(jobs)]]
            jobs.append((tr, te, X[tr].mean(axis=0), X[tr].std(axis=0), C))
    out = {"kind": np.array("svr_fit"), "X": X, "y": y, "kernel_type": np.array(smo_ref.KERNEL_TYPES[kernel]), "eps": np.array(eps),
           "epsilon": np.array(svr_fit_ref.SVR_EPSILON), "C": np.array([j[4] for j in jobs]), "mean": np.stack([j[2] for j in jobs]),
           "scale": np.stack([j[3] for j in jobs]),
           "train_off": np.concatenate([[0], np.cumsum([len(j[0]) for j in jobs])]).astype(np.int64),
           "test_off": np.concatenate([[0], np.cumsum([len(j[1]) for j in jobs])]).astype(np.int64),
           "train_idx": np.concatenate([j[0] for j in jobs]).astype(np.int32),
           "test_idx": np.concatenate([j[1] for j in jobs]).astype(np.int32)}
    preds, n_svs, tols, dists = [], [], [], []
    for j, job in enumerate(jobs):
        sk_pred, sk_n_sv, tol, dist = measure(X, y, job, kernel, eps, "%s job %d C=%g" % (kernel, j, job[4]))
        preds.append(sk_pred)
        n_svs.append(sk_n_sv)
        tols.append(tol)
        dists.append(dist)
    out.update({"sk_pred": np.concatenate(preds), "sk_n_sv": np.array(n_svs, dtype=np.int32), "tol_pred": np.array(tols),
                "distance": np.array(dists)})
    np.savez_compressed(os.path.join(OUT, "svr_fit_%s.npz" % kernel), **out)


if __name__ == "__main__":
    make("linear")
    make("rbf")
