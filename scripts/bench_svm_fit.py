#!/usr/bin/env python3
"""Times the SVM half of evaluate_classifier with svm_fit="device" (kernels_smo.hpp) on the shape extract_features_and_train
makes of 5 000 samples: 5 000 x 136, 8 classes, 7 values of C x int(50000 / 5000) + 1 = 11 experiments, for "svm" (linear) and
"svm_rbf".  Writes profiles/bench_svm_fit_n1_local.json.  Runs on the GPU.

Per kernel: the DEVICE time between two events on the library's stream around ONE svm_split_fit_predict call of the 77 jobs (the
solver's launches, the status read-backs between them, the vote kernel and the call's copies); the host-to-host time of
evaluate_classifier(svm_fit="device"); total and largest iteration count per task, the number of solver launches and the time
of one launch at the default budget (device time of a call stopped after one launch's worth of iterations, max_iter =
iters_per_launch, less nothing: uploads included, so an upper bound).  Beside them, where scikit-learn can be imported, the
scikit-learn loop on the same splits on this host's CPU, one thread, with probability=True (what the reference fits) and
probability=False (what the sweep reads), on --sklearn-jobs of the 77 jobs scaled up: a record, not a gate; null without
scikit-learn.

    python scripts/bench_svm_fit.py [--samples 5000] [--sklearn-jobs 3]
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PARAMS = [0.001, 0.01, 0.5, 1.0, 5.0, 10.0, 20.0]


def event_time(fn):
    """(device seconds between two events on the library stream around fn(), fn's return value)."""
    from pyaudioanalysis_amd import _ffi
    ms = ctypes.c_float()
    _ffi.check(_ffi.lib().paa_timer_start())
    ret = fn()
    _ffi.check(_ffi.lib().paa_timer_stop(ctypes.byref(ms)))
    return ms.value * 1e-3, ret


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--sklearn-jobs", type=int, default=3, help="jobs per kernel timed with scikit-learn (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_svm_fit_n1_local.json"))
    args = ap.parse_args()
    import train_ref
    from pyaudioanalysis_amd import _ffi, audioTrainTest as aT
    if _ffi.device_count() < 1:
        raise SystemExit("bench_svm_fit.py needs a HIP device")
    _ffi.init(0)
    feats = train_ref.bench_features(args.samples)
    X, y = train_ref.features_to_matrix(feats)
    n = X.shape[0]
    n_exp = int(50000 / n) + 1
    rng = np.random.default_rng(17)
    jobs = []
    for C in PARAMS:
        for _ in range(n_exp):
            perm = rng.permutation(n)
            tr, te = perm[:int(0.9 * n)], perm[int(0.9 * n):]
            jobs.append((tr, te, X[tr].mean(axis=0), X[tr].std(axis=0), C))
    geo = aT.smo_geometry()
    out = {"samples": n, "dims": X.shape[1], "classes": len(feats), "params": PARAMS, "n_exp": n_exp, "jobs": len(jobs),
           "iters_per_launch": geo[4], "threads_per_workgroup": geo[0], "kernels": {}}
    aT.svm_split_fit_predict(X, y, jobs[:1])                         # warm-up: library, lane scratch
    for kind, kernel in (("svm", "linear"), ("svm_rbf", "rbf")):
        rec = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rec["one_launch_at_default_budget_device_s"], one = event_time(
                lambda: aT.svm_split_fit_predict(X, y, jobs, kernel=kernel, max_iter=geo[4]))
        rec["one_launch_tasks_still_running"] = int(np.count_nonzero(one.status == aT.SMO_NOT_CONVERGED))
        print("%s: one launch %.3f s" % (kind, rec["one_launch_at_default_budget_device_s"]), file=sys.stderr, flush=True)
        rec["sweep_device_s"], res = event_time(lambda: aT.svm_split_fit_predict(X, y, jobs, kernel=kernel))
        print("%s: sweep %.3f s in %d launches" % (kind, rec["sweep_device_s"], res.n_launches), file=sys.stderr, flush=True)
        rec.update({"tasks": int(res.task_off[-1]), "iterations_total": int(res.iterations.sum()), "iterations_max": int(res.iterations.max()),
                    "iterations_median": float(np.median(res.iterations)), "solver_launches": res.n_launches,
                    "not_converged": int(np.count_nonzero(res.status == aT.SMO_NOT_CONVERGED)),
                    "support_vectors_per_task_mean": float(res.n_sv.mean()), "rows_per_task_mean": float(2 * 0.9 * n / len(feats)),
                    "accuracy_per_param": [float(np.mean(np.concatenate([res.job(p * n_exp + e)[0] == y[jobs[p * n_exp + e][1]]
                                                                         for e in range(n_exp)]))) for p in range(len(PARAMS))]})
        try:
            import sklearn  # noqa: F401
            np.random.seed(5)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                rec["evaluate_classifier_best_param"] = float(aT.evaluate_classifier(feats, ["c%d" % c for c in range(len(feats))], kind,
                                                                                     np.array(PARAMS), 1, svm_fit="device"))
            rec["evaluate_classifier_device_host_s"] = time.perf_counter() - t0
        except ImportError:
            rec["evaluate_classifier_device_host_s"] = None          # its splits and metrics are scikit-learn's
        rec["sklearn_probability_true_s"] = rec["sklearn_probability_false_s"] = None
        try:
            import sklearn.svm
            from threadpoolctl import threadpool_limits
            if args.sklearn_jobs > 0:
                pick = [jobs[(len(PARAMS) // 2) * n_exp + e] for e in range(args.sklearn_jobs)]      # C = 1
                with threadpool_limits(limits=1):
                    for prob in (True, False):
                        t0 = time.perf_counter()
                        agree = []
                        for p, (tr, te, mean, scale, C) in enumerate(pick):
                            clf = sklearn.svm.SVC(C=C, kernel=kernel, probability=prob, gamma="auto").fit((X[tr] - mean) / scale, y[tr])
                            agree.append(np.mean(clf.predict((X[te] - mean) / scale) == res.job((len(PARAMS) // 2) * n_exp + p)[0]))
                        per_job = (time.perf_counter() - t0) / len(pick)
                        print("%s: scikit-learn probability=%s %.2f s per job" % (kind, prob, per_job), file=sys.stderr, flush=True)
                        rec["sklearn_probability_%s_s" % str(prob).lower()] = per_job * len(jobs)
                rec["sklearn_jobs_timed"] = len(pick)
                rec["sklearn_note"] = "C = 1 jobs on one core, scaled to %d jobs" % len(jobs)
                rec["labels_equal_to_sklearn_share"] = float(np.mean(agree))
        except ImportError:
            pass
        out["kernels"][kind] = rec
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
