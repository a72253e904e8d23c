#!/usr/bin/env python3
"""Times the random-forest REGRESSOR fit on the GPU (kernels_treefit.hpp, K19) against scikit-learn on this host's CPU, one thread.
Writes profiles/bench_forest_reg_fit_n1_local.json.  Runs on the GPU.

Workload: the shape of scripts/bench_svr_fit.py, a seeded 2 000 x 136 matrix with a smooth target plus noise (its regression_data),
and the reference's grid of feature_extraction_train_regression, n_estimators = 5, 10, 25, 50, 100, x 10 experiments (the
reference runs 100; the time is linear in them) at 90 / 10: 50 splits of 1 800 training rows, 1 900 trees.
(a) the sweep: forest_regression_split_fit_predict on the 50 jobs with the training predictions, host to host (the host's per-tree
    NumPy draws included) and the DEVICE time between two events around the call; evaluate_regression(forest_fit="device") host to
    host (scaler, permutations, errors and the printed table included).
(b) scikit-learn on the SAME splits with the SAME seeds, one thread: a SAMPLE of the jobs -- the first experiment of n_estimators
    5, 10 and 25, 40 trees -- fitted and scored on test and training rows; its time per tree times 1 900 is the ESTIMATE of the
    full CPU sweep (--full-cpu runs all 50 jobs instead).  The targets are general, so there is no bit equality with scikit-learn
    (DESIGN K19); the record holds the largest absolute difference of the sampled jobs' test predictions and both mean squared
    errors instead.
(c) the final fit: train_random_forest_regression_device for 5, 25 and 100 trees on all 2 000 rows, host to host and device time,
    against scikit-learn's fit plus training prediction of the same forest (100 trees: estimated from the 25-tree fit unless
    --full-cpu).
A record, not a gate: slower cases are written down as they are.  The scikit-learn figures are null where it cannot be imported.

Every GPU time is the median of --repeats rounds after a warm-up, every single time beside it.

    python scripts/bench_forest_reg_fit.py [--samples 2000] [--n-exp 10] [--repeats 3] [--no-sklearn] [--full-cpu] [--out FILE]
"""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_forest_fit import event_time, host_time, quiet  # noqa: E402
from bench_svr_fit import regression_data  # noqa: E402

GRID = (5, 10, 25, 50, 100)
SAMPLE = (5, 10, 25)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--n-exp", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--full-cpu", action="store_true", help="fit all jobs and the 100-tree forest with scikit-learn too (minutes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_forest_reg_fit_n1_local.json"))
    args = ap.parse_args()
    from pyaudioanalysis_amd import _ffi, audioTrainTest as aT
    sklearn = None
    if not args.no_sklearn:
        try:
            import sklearn
            import sklearn.ensemble
            from threadpoolctl import threadpool_limits
        except ImportError:
            sklearn = None
    X, y = regression_data(args.samples)
    n, n_exp = X.shape[0], args.n_exp
    n_train = int(round(0.9 * n))
    rng = np.random.default_rng(17)
    jobs = []
    for ne in GRID:
        for _ in range(n_exp):
            perm = rng.permutation(n)
            tr, te = perm[:n_train], perm[n_train:]
            jobs.append((tr, te, X[tr].mean(0), X[tr].std(0), (ne, int(rng.integers(np.iinfo(np.int32).max)))))
    n_trees = sum(j[4][0] for j in jobs)
    rec = {"what": "random-forest regressor fit: GPU (one workgroup per tree, squared error, every feature at every node) against "
                   "scikit-learn on one CPU thread",
           "device": _ffi.device_name() if hasattr(_ffi, "device_name") else None, "samples": n, "dims": int(X.shape[1]), "grid": list(GRID),
           "n_exp": n_exp, "jobs": len(jobs), "train_rows": n_train, "trees_per_sweep": n_trees, "sklearn": getattr(sklearn, "__version__", None),
           "repeats": args.repeats}
    cpu = (lambda: threadpool_limits(limits=1)) if sklearn is not None else contextlib.nullcontext
    sweep = lambda: aT.forest_regression_split_fit_predict(X, y, jobs, train_pred=True)                # noqa: E731
    res = sweep()                                                                    # warm-up
    host, dev, full = [], [], []
    for _ in range(args.repeats):
        t, (d, res) = host_time(lambda: event_time(sweep))
        host.append(t)
        dev.append(d)
        np.random.seed(5)
        full.append(host_time(lambda: quiet(lambda: aT.evaluate_regression(X, y, n_exp, "randomforest", list(GRID), forest_fit="device")))[0])
    rec["sweep_host_s"], rec["sweep_host_s_all"] = float(np.median(host)), host
    rec["sweep_device_s"], rec["sweep_device_s_all"] = float(np.median(dev)), dev
    rec["evaluate_regression_host_s"], rec["evaluate_regression_host_s_all"] = float(np.median(full)), full
    rec["chunks"] = res.n_chunks
    if sklearn is not None:
        picked = list(range(len(jobs))) if args.full_cpu else [GRID.index(ne) * n_exp for ne in SAMPLE]
        t_cpu, diff, mse_gpu, mse_cpu = 0.0, 0.0, [], []
        with cpu():
            for j in picked:
                tr, te, mean, scale, (ne, seed) = jobs[j]
                t0 = time.perf_counter()
                m = sklearn.ensemble.RandomForestRegressor(n_estimators=ne, random_state=seed).fit((X[tr] - mean) / scale, y[tr])
                pred = m.predict((X[te] - mean) / scale)
                m.predict((X[tr] - mean) / scale)
                t_cpu += time.perf_counter() - t0
                diff = max(diff, float(np.max(np.abs(pred - res.job(j)[0]))))
                mse_cpu.append(float(np.mean((pred - y[te]) ** 2)))
                mse_gpu.append(float(np.mean((res.job(j)[0] - y[te]) ** 2)))
        cpu_trees = sum(jobs[j][4][0] for j in picked)
        rec["sklearn_jobs_fitted"], rec["sklearn_trees_fitted"], rec["sklearn_s"] = len(picked), cpu_trees, t_cpu
        rec["sklearn_sweep_s"], rec["sklearn_sweep_is_estimate"] = t_cpu * n_trees / cpu_trees, not args.full_cpu
        rec["max_abs_test_prediction_difference"], rec["test_mse_device"], rec["test_mse_sklearn"] = diff, mse_gpu, mse_cpu
        rec["sweep_speedup_host"] = rec["sklearn_sweep_s"] / rec["sweep_host_s"]
    print("sweep: %s" % json.dumps(rec), file=sys.stderr, flush=True)
    fits = {}
    for ne in (5, 25, 100):
        f = {}
        fit = lambda: aT.train_random_forest_regression_device(X, y, ne, random_state=7)      # noqa: E731
        arrays, _ = fit()
        host, dev = [], []
        for _ in range(args.repeats):
            t, (d, (arrays, err)) = host_time(lambda: event_time(fit))
            host.append(t)
            dev.append(d)
        f["host_s"], f["host_s_all"], f["device_s"], f["device_s_all"] = float(np.median(host)), host, float(np.median(dev)), dev
        f["nodes"], f["train_error"] = int(arrays.threshold.shape[0]), float(err)
        if sklearn is not None:
            ne_cpu = ne if (ne <= 25 or args.full_cpu) else 25

            def cpu_fit():
                m = sklearn.ensemble.RandomForestRegressor(n_estimators=ne_cpu, random_state=7).fit(X, y)
                return float(np.mean(np.abs(m.predict(X) - y)))
            with cpu():
                t, cpu_err = host_time(cpu_fit)
            f["sklearn_s"], f["sklearn_is_estimate"] = t * ne / ne_cpu, ne_cpu != ne
            if ne_cpu == ne:
                f["sklearn_train_error"] = cpu_err
            f["speedup_host"] = f["sklearn_s"] / f["host_s"]
        fits[str(ne)] = f
        print("train_random_forest_regression_device %d: %s" % (ne, json.dumps(f)), file=sys.stderr, flush=True)
    rec["train_random_forest_regression_device"] = fits
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
