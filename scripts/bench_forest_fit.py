#!/usr/bin/env python3
"""Times the random-forest / extra-trees fit on the GPU (kernels_treefit.hpp) against scikit-learn on this host's CPU, one thread.
Writes profiles/bench_forest_fit_n1_local.json.  Runs on the GPU.

Workload: the README's 5 000 x 136, 8-class set (tests/train_ref.bench_features) and the reference's grid, n_estimators = 10, 25,
50, 100, 200, 500 x n_exp = int(50000 / 5000) + 1 = 11 experiments at train_percentage 0.9: 66 splits of 4 500 training rows,
9 735 trees per kind ("randomforest", "extratrees").
(a) the sweep: forest_split_fit_predict on the 66 jobs, host to host (the host's per-tree NumPy draws included) and the DEVICE time
    between two events around the call; evaluate_classifier(forest_fit="device") host to host (splits, scalers, metrics and the
    printed table included).
(b) scikit-learn on the SAME splits with the SAME seeds, one thread: a SAMPLE of the jobs -- the first experiment of n_estimators
    10, 25 and 50, 85 trees -- fitted and scored; its time per tree times 9 735 is the estimate of the full CPU sweep (the full
    sweep is minutes long; --full-cpu runs all 66 jobs instead).  The sampled jobs' labels are compared with the sweep's: equal.
(c) the final fit: train_forest_device for 10, 100 and 500 trees on all 5 000 rows, host to host and device time, against
    scikit-learn's fit of the same forest (500 trees: estimated from the 100-tree fit unless --full-cpu).
A record, not a gate: slower cases are written down as they are.  The scikit-learn figures are null where it cannot be imported.

Every GPU time is the median of --repeats rounds after a warm-up, every single time beside it; rounds of the two modes alternate.

    python scripts/bench_forest_fit.py [--samples 5000] [--repeats 3] [--no-sklearn] [--full-cpu] [--out FILE]
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GRID = (10, 25, 50, 100, 200, 500)
SAMPLE = (10, 25, 50)


def event_time(fn):
    """(device seconds between two events on the library stream around fn(), fn's return value)."""
    from pyaudioanalysis_amd import _ffi
    ms = ctypes.c_float()
    _ffi.check(_ffi.lib().paa_timer_start())
    ret = fn()
    _ffi.check(_ffi.lib().paa_timer_stop(ctypes.byref(ms)))
    return ms.value * 1e-3, ret


def host_time(fn):
    t0 = time.perf_counter()
    ret = fn()
    return time.perf_counter() - t0, ret


def quiet(fn):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--full-cpu", action="store_true", help="fit all 66 jobs and the 500-tree forest with scikit-learn too (minutes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_forest_fit_n1_local.json"))
    args = ap.parse_args()
    import train_ref
    from pyaudioanalysis_amd import _ffi, audioTrainTest as aT
    sklearn = None
    if not args.no_sklearn:
        try:
            import sklearn
            import sklearn.ensemble
            from threadpoolctl import threadpool_limits
        except ImportError:
            sklearn = None
    feats = train_ref.bench_features(args.samples)
    names = ["c%d" % i for i in range(len(feats))]
    X, y = aT.features_to_matrix(feats)
    n = X.shape[0]
    n_exp = int(50000 / n) + 1
    np.random.seed(5)
    jobs = []
    for ne in GRID:
        for _ in range(n_exp):
            tr, te = aT._draw_split(n, 0.9)
            jobs.append((tr, te, X[tr].mean(0), X[tr].std(0), (ne, int(np.random.randint(np.iinfo(np.int32).max)))))
    n_trees = sum(j[4][0] for j in jobs)
    out = {"what": "random-forest / extra-trees fit: GPU (one workgroup per tree) against scikit-learn on one CPU thread",
           "device": _ffi.device_name() if hasattr(_ffi, "device_name") else None, "samples": n, "dims": int(X.shape[1]), "classes": len(feats),
           "grid": list(GRID), "n_exp": n_exp, "jobs": len(jobs), "train_rows": int(len(jobs[0][0])), "trees_per_sweep": n_trees,
           "sklearn": getattr(sklearn, "__version__", None), "repeats": args.repeats, "kinds": {}}
    cpu = (lambda: threadpool_limits(limits=1)) if sklearn is not None else contextlib.nullcontext
    for kind in ("randomforest", "extratrees"):
        rec = {}
        cls = None if sklearn is None else (sklearn.ensemble.RandomForestClassifier if kind == "randomforest" else sklearn.ensemble.ExtraTreesClassifier)
        sweep = lambda: aT.forest_split_fit_predict(X, y, jobs, kind)                # noqa: E731
        res = sweep()                                                                # warm-up
        host, dev, full = [], [], []
        for _ in range(args.repeats):
            t, (d, res) = host_time(lambda: event_time(sweep))
            host.append(t)
            dev.append(d)
            np.random.seed(5)
            full.append(host_time(lambda: quiet(lambda: aT.evaluate_classifier(feats, names, kind, list(GRID), 1, forest_fit="device")))[0])
        rec["sweep_host_s"], rec["sweep_host_s_all"] = float(np.median(host)), host
        rec["sweep_device_s"], rec["sweep_device_s_all"] = float(np.median(dev)), dev
        rec["evaluate_classifier_host_s"], rec["evaluate_classifier_host_s_all"] = float(np.median(full)), full
        rec["chunks"] = res.n_chunks
        if cls is not None:
            picked = list(range(len(jobs))) if args.full_cpu else [GRID.index(ne) * n_exp for ne in SAMPLE]
            t_cpu, equal = 0.0, True
            with cpu():
                for j in picked:
                    tr, te, mean, scale, (ne, seed) = jobs[j]
                    t0 = time.perf_counter()
                    m = cls(n_estimators=ne, random_state=seed).fit((X[tr] - mean) / scale, y[tr])
                    pred = m.predict((X[te] - mean) / scale)
                    t_cpu += time.perf_counter() - t0
                    equal &= bool(np.array_equal(pred, res.job(j)[0]))
            cpu_trees = sum(jobs[j][4][0] for j in picked)
            rec["sklearn_jobs_fitted"], rec["sklearn_trees_fitted"], rec["sklearn_s"] = len(picked), cpu_trees, t_cpu
            rec["sklearn_sweep_s"], rec["sklearn_sweep_is_estimate"] = t_cpu * n_trees / cpu_trees, not args.full_cpu
            rec["labels_equal_scikit_learn"] = equal
            rec["sweep_speedup_host"] = rec["sklearn_sweep_s"] / rec["sweep_host_s"]
        print("%s sweep: %s" % (kind, json.dumps(rec)), file=sys.stderr, flush=True)
        fits = {}
        for ne in (10, 100, 500):
            f = {}
            fit = lambda: aT.train_forest_device(X, y, ne, kind, random_state=7)      # noqa: E731
            arrays = fit()
            host, dev = [], []
            for _ in range(args.repeats):
                t, (d, arrays) = host_time(lambda: event_time(fit))
                host.append(t)
                dev.append(d)
            f["host_s"], f["host_s_all"], f["device_s"], f["device_s_all"] = float(np.median(host)), host, float(np.median(dev)), dev
            f["nodes"] = int(arrays.threshold.shape[0])
            if cls is not None:
                ne_cpu = ne if (ne <= 100 or args.full_cpu) else 100
                with cpu():
                    t, m = host_time(lambda: cls(n_estimators=ne_cpu, random_state=7).fit(X, y))
                f["sklearn_s"], f["sklearn_is_estimate"] = t * ne / ne_cpu, ne_cpu != ne
                if ne_cpu == ne:
                    f["arrays_equal_scikit_learn"] = bool(aT.forest_arrays(m).threshold.tobytes() == arrays.threshold.tobytes())
                f["speedup_host"] = f["sklearn_s"] / f["host_s"]
            fits[str(ne)] = f
            print("%s train_forest_device %d: %s" % (kind, ne, json.dumps(f)), file=sys.stderr, flush=True)
        rec["train_forest_device"] = fits
        out["kinds"][kind] = rec
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
