#!/usr/bin/env python3
"""Times the SVR half of evaluate_regression with svm_fit="device" (kernels_svrfit.hpp) on the shape
feature_extraction_train_regression makes of 2 000 files: a seeded 2 000 x 136 matrix with a smooth target plus noise, the
reference's 10 values of C x 100 experiments, for "svm" (linear) and "svm_rbf".  Writes profiles/bench_svr_fit_n1_local.json.
Runs on the GPU.

Per kernel: the DEVICE time between two events on the library's stream around ONE svr_split_fit_predict call of all jobs (the
solver's launches, the status read-backs between them, the scoring kernel and the call's copies); the host-to-host time of
evaluate_regression(svm_fit="device"); the iteration counts per task (maximum, median, total; per value of C the maximum) and
the number of solver launches.  Beside them, where scikit-learn can be imported, SVR fits on the same splits on this host's
CPU, one thread, on --sklearn-jobs jobs per value of C, scaled to the sweep: a record, not a gate; null without scikit-learn.
--n-exp and --max-iter shorten a run; the record says what ran.  evaluate_regression has no iteration cap, so with --max-iter
below libsvm's 10^7 its timing is skipped for a kernel whose capped sweep left tasks unconverged (null in the record).  No
speed-up is promised by this script: it states what was measured.

    python scripts/bench_svr_fit.py [--samples 2000] [--n-exp 100] [--sklearn-jobs 1]

--cache compares the resident kernel matrix (kernel_cache="gram", kernels_svrcache.hpp) with the recomputing solver
(kernel_cache="none") instead and writes profiles/bench_svr_cache_n1_local.json: per kernel and mode the device time of the
sweep and of the final fit (ONE task over all samples at the value of C with the least test error of the sweep, what
train_svm_regression_device solves), medians of --rounds rounds after a warm-up; the same sweep with max_iter = 1 under "gram"
(uploads, the standardise and Gram kernels, one iteration, scoring: an upper bound of the Gram pass's share); whether the two
modes returned the same bytes; scikit-learn on one core on one split per value of C, under the same iteration cap.

    python scripts/bench_svr_fit.py --cache --n-exp 10 --max-iter 200000
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)
from bench_svm_fit import event_time  # noqa: E402

PARAMS = [0.001, 0.005, 0.01, 0.05, 0.1, 0.25, 0.5, 1.0, 5.0, 10.0]     # feature_extraction_train_regression's values of C
DIMS = 136


def regression_data(n, seed=23):
    """(X [n][136] on features of unequal scale and offset, y [n]: a smooth function of three directions plus noise)."""
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((n, DIMS))
    w = rng.standard_normal((3, DIMS)) / np.sqrt(DIMS)
    y = 2.0 + np.tanh(U @ w[0]) + 0.5 * (U @ w[1]) + 0.3 * np.sin(2.0 * (U @ w[2])) + 0.1 * rng.standard_normal(n)
    return U * rng.uniform(0.5, 3.0, DIMS) + rng.uniform(-2.0, 2.0, DIMS), y


def cache_compare(args, aT, Z, y, jobs):
    """The --cache record (see the module docstring)."""
    n = Z.shape[0]
    geo = aT.smo_geometry()
    out = {"samples": n, "dims": DIMS, "params": PARAMS, "n_exp": args.n_exp, "jobs": len(jobs), "rows_per_task": len(jobs[0][0]),
           "max_iter": args.max_iter, "iters_per_launch": geo[4], "rounds": args.rounds, "cache_bytes": aT.SVR_CACHE_BYTES,
           "matrix_bytes_per_task": 8 * len(jobs[0][0]) ** 2, "kernels": {}}

    def save():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    def timed(fn, slow_s=120.0):
        """(median device seconds, every round, the last result): --rounds rounds, one when the first takes longer than slow_s."""
        times, res = [], None
        for _ in range(args.rounds):
            t, res = event_time(fn)
            times.append(t)
            if t > slow_s:
                break
        return float(np.median(times)), times, res

    all_rows, zeros, ones = np.arange(n), np.zeros(DIMS), np.ones(DIMS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for mode in ("none", "gram"):                    # warm-up: library, lane scratch, both solvers' code
            aT.svr_split_fit_predict(Z, y, jobs[:2], max_iter=10, kernel_cache=mode)
        for kind in args.kinds.split(","):
            kernel = "rbf" if kind == "svm_rbf" else "linear"
            rec = {}
            out["kernels"][kind] = rec
            sweeps = {}
            for mode in ("gram", "none"):
                med, times, res = timed(lambda: aT.svr_split_fit_predict(Z, y, jobs, kernel=kernel, train_pred=True, max_iter=args.max_iter,
                                                                         kernel_cache=mode))
                sweeps[mode] = res
                rec["sweep_%s_device_s" % mode], rec["sweep_%s_rounds_s" % mode] = med, times
                print("%s %s: sweep %.3f s (%d rounds), %d launches" % (kind, mode, med, len(times), res.n_launches), file=sys.stderr, flush=True)
                save()
            a, b = sweeps["none"], sweeps["gram"]
            rec["sweep_bytes_equal"] = bool(a.pred.tobytes() == b.pred.tobytes() and a.train_pred.tobytes() == b.train_pred.tobytes() and
                                            np.array_equal(a.iterations, b.iterations) and np.array_equal(a.n_sv, b.n_sv))
            rec.update({"tasks_cached": int(b.cached.sum()), "iterations_total": int(b.iterations.sum()), "iterations_max": int(b.iterations.max()),
                        "not_converged": int(np.count_nonzero(b.status == aT.SMO_NOT_CONVERGED)), "solver_launches": b.n_launches})
            rec["sweep_gram_max_iter_1_device_s"], rec["sweep_gram_max_iter_1_rounds_s"], _ = timed(
                lambda: aT.svr_split_fit_predict(Z, y, jobs, kernel=kernel, train_pred=True, max_iter=1, kernel_cache="gram"))
            rec["gram_pass_share_of_sweep_at_most"] = rec["sweep_gram_max_iter_1_device_s"] / rec["sweep_gram_device_s"]
            rec["sweep_speedup_gram_over_none"] = rec["sweep_none_device_s"] / rec["sweep_gram_device_s"]
            # the sweep lasts as long as its longest task: its time over that task's iterations bounds the time per iteration from above
            rec["device_us_per_iteration_of_the_longest_task_none"] = 1e6 * rec["sweep_none_device_s"] / rec["iterations_max"]
            rec["device_us_per_iteration_of_the_longest_task_gram"] = 1e6 * rec["sweep_gram_device_s"] / rec["iterations_max"]
            mse = [float(np.mean([np.mean((b.job(p * args.n_exp + e)[0] - y[jobs[p * args.n_exp + e][1]]) ** 2) for e in range(args.n_exp)]))
                   for p in range(len(PARAMS))]
            C = PARAMS[int(np.argmin(mse))]
            gamma = 1.0 / (DIMS * Z.var()) if kernel == "rbf" else 1.0
            rec["final_fit_C"], rec["final_fit_rows"] = C, n
            fits = {}
            for mode in ("gram", "none"):
                med, times, fits[mode] = timed(lambda: aT.svr_solve(Z, y, [(all_rows, zeros, ones, C, gamma, 0.1)], kernel=kernel,
                                                                    max_iter=args.max_iter, kernel_cache=mode))
                rec["final_fit_%s_device_s" % mode], rec["final_fit_%s_rounds_s" % mode] = med, times
            rec["final_fit_iterations"] = int(fits["gram"].iterations[0])
            rec["final_fit_bytes_equal"] = bool(fits["gram"].beta[0].tobytes() == fits["none"].beta[0].tobytes() and
                                                fits["gram"].rho.tobytes() == fits["none"].rho.tobytes())
            rec["final_fit_speedup_gram_over_none"] = rec["final_fit_none_device_s"] / rec["final_fit_gram_device_s"]
            save()
            rec["sklearn_sweep_s"] = rec["sklearn_final_fit_s"] = None
            try:
                import sklearn.svm
                from threadpoolctl import threadpool_limits
                with threadpool_limits(limits=1):
                    per_param = []
                    for p, Cp in enumerate(PARAMS):
                        tr, te = jobs[p * args.n_exp][:2]
                        t0 = time.perf_counter()
                        sklearn.svm.SVR(C=Cp, kernel=kernel, max_iter=args.max_iter).fit(Z[tr], y[tr]).predict(Z[te])
                        per_param.append(time.perf_counter() - t0)
                        print("%s: scikit-learn C=%g %.2f s" % (kind, Cp, per_param[-1]), file=sys.stderr, flush=True)
                    t0 = time.perf_counter()
                    sklearn.svm.SVR(C=C, kernel=kernel, max_iter=args.max_iter).fit(Z, y)
                    rec["sklearn_final_fit_s"] = time.perf_counter() - t0
                rec["sklearn_s_per_fit_per_param"] = per_param
                rec["sklearn_sweep_s"] = float(np.sum(per_param) * args.n_exp)
                rec["sklearn_note"] = ("one fit + predict per value of C on one core under max_iter = %d, scaled to %d experiments; one "
                                       "round" % (args.max_iter, args.n_exp))
            except ImportError:
                pass
            save()
    out["note"] = args.note
    save()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--n-exp", type=int, default=100)
    ap.add_argument("--max-iter", type=int, default=10**7)
    ap.add_argument("--kinds", default="svm_rbf,svm")
    ap.add_argument("--sklearn-jobs", type=int, default=1, help="jobs per value of C timed with scikit-learn (0: none)")
    ap.add_argument("--no-evaluate", action="store_true", help="skip the evaluate_regression(svm_fit='device') timing")
    ap.add_argument("--cache", action="store_true", help="compare kernel_cache='gram' with 'none' (see above)")
    ap.add_argument("--rounds", type=int, default=3, help="--cache: timed rounds per figure (the median is recorded)")
    ap.add_argument("--note", default="", help="--cache: a note kept in the record")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "bench_svr_cache_n1_local.json" if args.cache else "bench_svr_fit_n1_local.json")
    from pyaudioanalysis_amd import _ffi, audioTrainTest as aT
    if _ffi.device_count() < 1:
        raise SystemExit("bench_svr_fit.py needs a HIP device")
    _ffi.init(0)
    X, y = regression_data(args.samples)
    n = X.shape[0]
    Z = (X - X.mean(axis=0)) / X.std(axis=0)            # evaluate_regression standardises once, before the splits
    n_train = int(round(0.9 * n))
    zeros, ones = np.zeros(DIMS), np.ones(DIMS)
    rng = np.random.default_rng(17)
    jobs = []
    for C in PARAMS:
        for _ in range(args.n_exp):
            perm = rng.permutation(n)
            jobs.append((perm[:n_train], perm[n_train:], zeros, ones, C))
    if args.cache:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        return cache_compare(args, aT, Z, y, jobs)
    geo = aT.smo_geometry()
    out = {"samples": n, "dims": DIMS, "params": PARAMS, "n_exp": args.n_exp, "jobs": len(jobs), "rows_per_task": n_train,
           "max_iter": args.max_iter, "iters_per_launch": geo[4], "threads_per_workgroup": geo[0], "kernels": {}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        aT.svr_split_fit_predict(Z, y, jobs[:1], max_iter=10)          # warm-up: library, lane scratch
    for kind in args.kinds.split(","):
        kernel = "rbf" if kind == "svm_rbf" else "linear"
        rec = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rec["sweep_device_s"], res = event_time(lambda: aT.svr_split_fit_predict(Z, y, jobs, kernel=kernel, train_pred=True,
                                                                                     max_iter=args.max_iter))
        print("%s: sweep %.3f s in %d launches, at most %d iterations" % (kind, rec["sweep_device_s"], res.n_launches, res.iterations.max()),
              file=sys.stderr, flush=True)
        its = res.iterations.reshape(len(PARAMS), args.n_exp)
        mse = [float(np.mean([np.mean((res.job(p * args.n_exp + e)[0] - y[jobs[p * args.n_exp + e][1]]) ** 2) for e in range(args.n_exp)]))
               for p in range(len(PARAMS))]
        rec.update({"tasks": len(jobs), "iterations_total": int(res.iterations.sum()), "iterations_max": int(res.iterations.max()),
                    "iterations_median": float(np.median(res.iterations)), "iterations_max_per_param": its.max(axis=1).tolist(),
                    "solver_launches": res.n_launches, "not_converged": int(np.count_nonzero(res.status == aT.SMO_NOT_CONVERGED)),
                    "support_vectors_per_task_mean": float(res.n_sv.mean()), "test_mse_per_param": mse})
        out["kernels"][kind] = rec
        save()
        rec["evaluate_regression_device_host_s"] = rec["evaluate_regression_best_param"] = None
        if not args.no_evaluate and rec["not_converged"] == 0:         # (an uncapped run of tasks the cap stopped can take very long)
            try:
                import sklearn  # noqa: F401  (its StandardScaler is evaluate_regression's)
                np.random.seed(5)
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    rec["evaluate_regression_best_param"] = float(aT.evaluate_regression(X, y, args.n_exp, kind, np.array(PARAMS),
                                                                                         svm_fit="device")[0])
                rec["evaluate_regression_device_host_s"] = time.perf_counter() - t0
            except ImportError:
                pass
        rec["sklearn_s"] = None
        try:
            import sklearn.svm
            from threadpoolctl import threadpool_limits
            if args.sklearn_jobs > 0:
                per_param, dist = [], []
                with threadpool_limits(limits=1):
                    for p, C in enumerate(PARAMS):
                        t0 = time.perf_counter()
                        for e in range(args.sklearn_jobs):
                            tr, te = jobs[p * args.n_exp + e][:2]
                            svr = sklearn.svm.SVR(C=C, kernel=kernel).fit(Z[tr], y[tr])
                            dist.append(float(np.max(np.abs(svr.predict(Z[te]) - res.job(p * args.n_exp + e)[0]))))
                        per_param.append((time.perf_counter() - t0) / args.sklearn_jobs)
                        print("%s: scikit-learn C=%g %.2f s per fit" % (kind, C, per_param[-1]), file=sys.stderr, flush=True)
                rec["sklearn_s_per_fit_per_param"] = per_param
                rec["sklearn_s"] = float(np.sum(per_param) * args.n_exp)
                rec["sklearn_note"] = "%d fit(s) + predict per value of C on one core, scaled to %d experiments" % (args.sklearn_jobs, args.n_exp)
                rec["max_abs_distance_to_sklearn_predictions"] = float(np.max(dist))
        except ImportError:
            pass
        save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
