#!/usr/bin/env python3
"""Times the gradient-boosting fit on the GPU (kernels_boost.hpp, the Friedman instance of kernels_treefit.hpp, lib_boost.hpp) against
scikit-learn on this host's CPU, one thread.  Writes profiles/bench_boost_fit_n1_local.json.  Runs on the GPU.

Workload: the README's 5 000 x 136, 8-class set (tests/train_ref.bench_features) and the reference's grid, n_estimators = 10, 25,
50, 100, 200, 500 x n_exp = int(50000 / 5000) + 1 = 11 experiments at train_percentage 0.9: 66 splits of 4 500 training rows,
9 735 stages, 77 880 trees.
(a) the sweep: boosting_split_fit_predict on the 66 jobs, host to host and the DEVICE time between two events around the call;
    evaluate_classifier(boosting_fit="device") host to host (splits, scalers, metrics and the printed table included); the time per
    stage = device time / 500, the number of stage launches of the sweep (the jobs of a stage run side by side).
(b) scikit-learn on the SAME splits with the SAME seeds, one thread: a SAMPLE -- the first experiment of n_estimators 10, fitted and
    scored; its time per tree times 77 880 is the ESTIMATE of the full CPU sweep (hours long; --cpu-stages picks another sample).
    The first stages are the dearest (full depth-3 trees; later stages may close nodes early), so scaling from them probably
    OVERSTATES scikit-learn's cost; the record marks every scaled figure.
(c) the final fit: train_gradient_boosting_device for 10, 100 and 500 stages on all 5 000 rows, host to host and device time,
    against scikit-learn's fit scaled by trees from --cpu-stages stages (the figures say which are scaled).
(d) the share of the gradient kernel: --kernel-stats FILE folds the per-kernel totals of a `rocprofv3 --kernel-trace --stats` run of
    `bench_boost_fit.py --sweep-only` (the warm-up sweep and one more, nothing timed) into the record.
A record, not a gate: slower cases are written down as they are.  The scikit-learn figures are null where it cannot be imported.
Every GPU time is the median of --repeats rounds after a warm-up, every single time beside it.

    python scripts/bench_boost_fit.py [--samples 5000] [--repeats 3] [--no-sklearn] [--cpu-stages 10] [--kernel-stats CSV] [--out FILE]
"""
import argparse
import contextlib
import csv
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


def kernel_shares(path):
    """Per kernel the total nanoseconds and calls of a rocprofv3 kernel_stats.csv, and the share of the boosting kernels."""
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {"source": "rocprofv3 --kernel-trace --stats of bench_boost_fit.py --sweep-only (two sweeps); the trace itself is not kept in the repository",
           "total_kernel_s": total * 1e-9, "kernels": {}}
    for r in rows:
        name = r["Name"]
        key = "gradient" if "boost_gradient_kernel" in name else "trees" if "tree_fit_kernel" in name else "predict" if "forest_" in name else \
            "prep" if "tree_prep" in name or "tree_gather" in name else None
        if key:
            k = out["kernels"].setdefault(key, {"s": 0.0, "calls": 0})
            k["s"] += float(r["TotalDurationNs"]) * 1e-9
            k["calls"] += int(r["Calls"])
    for k in out["kernels"].values():
        k["share"] = k["s"] * 1e9 / total if total else None
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--cpu-stages", type=int, default=10, help="stages of the scikit-learn fits that the CPU figures are scaled from")
    ap.add_argument("--sweep-only", action="store_true", help="one warm-up and one sweep, nothing timed or written (for a kernel trace)")
    ap.add_argument("--kernel-stats", help="a rocprofv3 kernel_stats.csv of a --sweep-only run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_boost_fit_n1_local.json"))
    args = ap.parse_args()
    import train_ref
    from pyaudioanalysis_amd import audioTrainTest as aT
    shares = kernel_shares(args.kernel_stats) if args.kernel_stats else None          # (read first: a wrong path ends the run here)
    sklearn = None
    if not args.no_sklearn and not args.sweep_only:
        try:
            import sklearn
            import sklearn.ensemble
            from threadpoolctl import threadpool_limits
        except ImportError:
            sklearn = None
    feats = train_ref.bench_features(args.samples)
    names = ["c%d" % i for i in range(len(feats))]
    X, y = aT.features_to_matrix(feats)
    n, K = X.shape[0], len(feats)
    n_exp = int(50000 / n) + 1
    np.random.seed(5)
    jobs = []
    for ne in GRID:
        for _ in range(n_exp):
            tr, te = aT._draw_split(n, 0.9)
            jobs.append((tr, te, X[tr].mean(0), X[tr].std(0), (ne, int(np.random.randint(np.iinfo(np.int32).max)))))
    n_stages = sum(j[4][0] for j in jobs)
    sweep = lambda: aT.boosting_split_fit_predict(X, y, jobs)                        # noqa: E731
    res = sweep()                                                                    # warm-up
    if args.sweep_only:
        sweep()
        return
    out = {"what": "gradient-boosting fit: GPU (per stage a gradient launch and a tree launch, one workgroup per (job, class) tree) against "
                   "scikit-learn on one CPU thread",
           "samples": n, "dims": int(X.shape[1]), "classes": K, "grid": list(GRID), "n_exp": n_exp, "jobs": len(jobs),
           "train_rows": int(len(jobs[0][0])), "stages_per_sweep": n_stages, "trees_per_sweep": n_stages * K,
           "sklearn": getattr(sklearn, "__version__", None), "repeats": args.repeats}
    cpu = (lambda: threadpool_limits(limits=1)) if sklearn is not None else contextlib.nullcontext
    rec = {}
    host, dev, full = [], [], []
    for _ in range(args.repeats):
        t, (d, res) = host_time(lambda: event_time(sweep))
        host.append(t)
        dev.append(d)
        np.random.seed(5)
        full.append(host_time(lambda: quiet(lambda: aT.evaluate_classifier(feats, names, "gradientboosting", list(GRID), 1, boosting_fit="device")))[0])
    rec["sweep_host_s"], rec["sweep_host_s_all"] = float(np.median(host)), host
    rec["sweep_device_s"], rec["sweep_device_s_all"] = float(np.median(dev)), dev
    rec["evaluate_classifier_host_s"], rec["evaluate_classifier_host_s_all"] = float(np.median(full)), full
    rec["chunks"], rec["stage_launches"] = res.n_chunks, max(GRID) * res.n_chunks
    rec["device_s_per_stage_launch"] = rec["sweep_device_s"] / rec["stage_launches"]
    if sklearn is not None:
        j = 0                                                                        # the first experiment of n_estimators = 10
        tr, te, mean, scale, (ne, seed) = jobs[j]
        with cpu():
            t_cpu, m = host_time(lambda: sklearn.ensemble.GradientBoostingClassifier(n_estimators=args.cpu_stages, random_state=seed).fit((X[tr] - mean) / scale, y[tr]))
            pred = m.predict((X[te] - mean) / scale)
        rec["sklearn_stages_fitted"], rec["sklearn_s"] = args.cpu_stages, t_cpu
        rec["sklearn_sweep_s"], rec["sklearn_sweep_is_estimate"] = t_cpu * n_stages / args.cpu_stages, True
        if args.cpu_stages == ne:
            rec["held_out_labels_equal_scikit_learn"] = float(np.mean(pred == res.job(j)[0]))
        rec["sweep_speedup_host"] = rec["sklearn_sweep_s"] / rec["sweep_host_s"]
    print("sweep: %s" % json.dumps(rec), file=sys.stderr, flush=True)
    fits = {}
    for ne in (10, 100, 500):
        f = {}
        fit = lambda: aT.train_gradient_boosting_device(X, y, ne, random_state=7)     # noqa: E731
        model = fit()
        host, dev = [], []
        for _ in range(args.repeats):
            t, (d, model) = host_time(lambda: event_time(fit))
            host.append(t)
            dev.append(d)
        f["host_s"], f["host_s_all"], f["device_s"], f["device_s_all"] = float(np.median(host)), host, float(np.median(dev)), dev
        f["device_s_per_stage"] = f["device_s"] / ne
        f["nodes"], f["train_score_last"] = int(model.threshold.shape[0]), float(model.train_score_[-1])
        if sklearn is not None:
            with cpu():
                t, m = host_time(lambda: sklearn.ensemble.GradientBoostingClassifier(n_estimators=args.cpu_stages, random_state=7).fit(X, y))
            f["sklearn_s"], f["sklearn_is_estimate"] = t * ne / args.cpu_stages, ne != args.cpu_stages
            if ne == args.cpu_stages:
                f["train_score_last_scikit_learn"] = float(m.train_score_[-1])
            f["speedup_host"] = f["sklearn_s"] / f["host_s"]
        fits[str(ne)] = f
        print("train_gradient_boosting_device %d: %s" % (ne, json.dumps(f)), file=sys.stderr, flush=True)
    rec["train_gradient_boosting_device"] = fits
    out["gradientboosting"] = rec
    if shares is not None:
        out["kernel_shares_of_traced_sweeps"] = shares
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
