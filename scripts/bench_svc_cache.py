#!/usr/bin/env python3
"""Times the C-SVC fits with and without resident kernel matrices (kernel_cache="gram", DESIGN K23: kernels_smocache.hpp) and
writes profiles/bench_svc_cache_n1_local.json.  Runs on the GPU.

"none" and "gram" alternate in one process, host -> host, medians of --repeats rounds after a warm-up, on the configurations of
  scripts/bench_svm_fit.py        the 77-split sweep of 5 000 x 136, 8 classes, linear and RBF (svm_split_fit_predict)
  scripts/bench_platt.py          train_svm_device 5 000 x 136, linear and RBF, against scikit-learn in the same rounds (one core);
                                  silence_removal(svm_fit="device") of a 20 s and a 3 min clip
  scripts/bench_silence_batch.py  silence_removal_batch of 200 x 20 s and 50 x 3 min
Per configuration: the total time of either mode; the Gram pass (the difference of the two modes when both stop after ONE
iteration per task, max_iter = 1: what "gram" adds before its first iteration; not available where no entry point takes max_iter,
there the fits' stage times stand for it) and its share of the "gram" total; the time of one solver iteration of the
configuration's longest task solved ALONE, one workgroup, either mode (the slope between two iteration caps); the number of chunks
and the peak bytes of resident matrices under the budget (audioTrainTest.smo_cache_layout's rule on the jobs' row counts).

--parent times the "none" configurations only and passes no keyword the parent commit lacks: run it on a build of the parent
(--package-root: the directory that holds that build's pyaudioanalysis_amd) to see that the untouched path did not move.

    python scripts/bench_svc_cache.py [--repeats 5] [--parent --package-root DIR --out FILE]
"""
import argparse
import contextlib
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 16000
PARAMS = [0.001, 0.01, 0.5, 1.0, 5.0, 10.0, 20.0]


def timed(fn):
    t0 = time.perf_counter()
    ret = fn()
    return time.perf_counter() - t0, ret


def alternate(fns, repeats):
    """({name: median seconds}, {name: every time}, {name: last return value}) of the calls of fns, timed alternately after one
    warm-up round (every call ends in a device synchronise or runs on the CPU)."""
    times, last = {k: [] for k in fns}, {}
    for r in range(repeats + 1):
        for k, fn in fns.items():
            np.random.seed(5)
            t, last[k] = timed(fn)
            if r:
                times[k].append(t)
    return {k: float(np.median(v)) for k, v in times.items()}, times, last


def layout(row_counts, budget):
    """(chunks, peak bytes of one chunk, groups not cached) for groups of these row counts under the packing rule."""
    from pyaudioanalysis_amd import audioTrainTest as aT
    chunk = aT.svr_cache_chunks(row_counts, budget)
    sizes = np.array([8 * int(n) * int(n) for n in row_counts])
    peak = max((int(sizes[chunk == c].sum()) for c in range(int(chunk.max()) + 1)), default=0)
    return int(chunk.max()) + 1, peak, int(np.count_nonzero(chunk < 0))


def iteration_us(aT, X, task, kernel, modes):
    """{mode: microseconds per iteration} of one task solved alone: the slope between max_iter = lo and hi (both below its stop)."""
    full = aT.smo_solve(X, [task], kernel=kernel)
    hi = int(min(full.iterations[0], 4000))
    lo = max(1, hi // 4)
    out = {"task_rows": int(len(task[0])), "task_iterations": int(full.iterations[0]), "between_iterations": [lo, hi]}
    if hi <= lo:
        return out
    for mode in modes:
        kw = {} if mode == "none" else dict(kernel_cache="gram")
        med, _, _ = alternate({"lo": lambda: aT.smo_solve(X, [task], kernel=kernel, max_iter=lo, **kw),
                               "hi": lambda: aT.smo_solve(X, [task], kernel=kernel, max_iter=hi, **kw)}, 5)
        out[mode] = 1e6 * (med["hi"] - med["lo"]) / (hi - lo)
    return out


def base_clip(k):
    from synth import synth_clip
    x = synth_clip(700 + k, 20 * FS).copy()
    rng = np.random.default_rng(3 + k)
    for _ in range(8):                                  # digital silence between bursts
        a = int(rng.integers(0, 19 * FS))
        x[a:a + int(rng.integers(FS // 4, FS))] = 0
    return x


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--short", type=int, default=200, help="clips of 20 s in the batch")
    ap.add_argument("--long", type=int, default=50, help="clips of 3 min in the batch")
    ap.add_argument("--parent", action="store_true", help='"none" only, without the new keywords')
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_svc_cache_n1_local.json"))
    args = ap.parse_args()
    for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.abspath(args.package_root)):
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)
    import train_ref
    from pyaudioanalysis_amd import ShortTermFeatures as stf, _ffi, audioSegmentation as aS, audioTrainTest as aT
    if _ffi.device_count() < 1:
        raise SystemExit("bench_svc_cache.py needs a HIP device")
    _ffi.init(0)
    try:
        if args.no_sklearn:
            raise ImportError
        import sklearn.svm
        from threadpoolctl import threadpool_limits
        one_core = lambda: threadpool_limits(limits=1)      # noqa: E731
    except ImportError:
        sklearn, one_core = None, contextlib.nullcontext
    warnings.simplefilter("ignore")
    modes = ("none",) if args.parent else ("none", "gram")
    cache = {"none": {}, "gram": dict(kernel_cache="gram")}
    budget = getattr(aT, "SVR_CACHE_BYTES", 4 << 30)
    out = {"package": os.path.dirname(os.path.abspath(aT.__file__)), "modes": list(modes), "repeats": args.repeats, "cache_bytes": budget,
           "configurations": {}}

    def record(name, rec):
        if "gram_s" in rec:
            rec["gram_over_none"] = rec["none_s"] / rec["gram_s"]
            if rec.get("gram_pass_s") is not None:
                rec["gram_pass_share_of_gram_total"] = rec["gram_pass_s"] / rec["gram_s"]
        print("%s: %s" % (name, json.dumps({k: v for k, v in rec.items() if not k.endswith("_all")})), file=sys.stderr, flush=True)
        out["configurations"][name] = rec

    def gram_pass(call):
        """the difference of the two modes of call(max_iter=1, **keywords), medians of alternating rounds"""
        if args.parent:
            return None
        med, _, _ = alternate({m: (lambda m=m: call(max_iter=1, **cache[m])) for m in modes}, args.repeats)
        return med["gram"] - med["none"]

    # (a) the sweep
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
    for kind, kernel in (("svm", "linear"), ("svm_rbf", "rbf")):
        call = lambda **kw: aT.svm_split_fit_predict(X, y, jobs, kernel=kernel, **kw)      # noqa: E731
        med, every, last = alternate({m: (lambda m=m: call(**cache[m])) for m in modes}, args.repeats)
        res = last["none"]
        rec = {"jobs": len(jobs), "rows_per_job": int(len(jobs[0][0])), "tasks": int(res.task_off[-1]), "iterations_max": int(res.iterations.max()),
               "iterations_total": int(res.iterations.sum()), "solver_launches": {m: last[m].n_launches for m in modes}}
        rec.update({m + "_s": med[m] for m in modes})
        rec.update({m + "_s_all": every[m] for m in modes})
        if not args.parent:
            rec["same_labels"] = bool(np.array_equal(last["gram"].label, res.label))
            rec["jobs_cached"] = int(np.count_nonzero(last["gram"].cached))
        rec["gram_pass_s"] = gram_pass(call)
        rec["chunks"], rec["peak_cache_bytes"], rec["groups_not_cached"] = layout([len(j[0]) for j in jobs], budget)
        # the longest task of the C = 20 jobs, alone
        j = len(jobs) - 1
        t = int(np.argmax(res.iterations[res.task_off[j]:res.task_off[j + 1]]))
        cl = res.classes[j]
        pairs = [(a, b) for a in range(len(cl)) for b in range(a + 1, len(cl))]
        tr, lab = jobs[j][0], y[jobs[j][0]]
        ra, rb = tr[lab == cl[pairs[t][0]]], tr[lab == cl[pairs[t][1]]]
        task = (np.concatenate([ra, rb]), np.concatenate([np.ones(len(ra)), -np.ones(len(rb))]), jobs[j][2], jobs[j][3], jobs[j][4], None)
        rec["iteration_us_one_task_alone"] = iteration_us(aT, X, task, kernel, modes)
        record("sweep_" + kind, rec)

    # (b) train_svm_device against scikit-learn
    Z = (X - X.mean(axis=0)) / X.std(axis=0)
    for kind, kernel in (("svm", "linear"), ("svm_rbf", "rbf")):
        fns = {m: (lambda m=m: aT.train_svm_device(Z, y, 1.0, kernel, random_state=3, **cache[m])) for m in modes}
        if sklearn is not None:
            fns["sklearn"] = lambda: sklearn.svm.SVC(C=1.0, kernel=kernel, probability=True, gamma="auto", random_state=3).fit(Z, y)
        with one_core():
            med, every, last = alternate(fns, args.repeats)
        fit = last["none"].fit_result
        rec = {"rows": n, "pairs": len(fit.rows), "tasks": int(np.count_nonzero(fit.status)), "iterations_max": int(fit.iterations.max()),
               "iterations_total": int(fit.iterations.sum()), "solver_launches": {m: last[m].fit_result.n_launches for m in modes},
               "sklearn_s": med.get("sklearn"), "sklearn_note": "one core of the GPU host, the same rounds"}
        rec.update({m + "_s": med[m] for m in modes})
        rec.update({k + "_s_all": v for k, v in every.items()})
        if not args.parent:
            rec["same_model"] = bool(last["gram"].probA_.tobytes() == last["none"].probA_.tobytes()
                                     and last["gram"]._dual_coef_.tobytes() == last["none"]._dual_coef_.tobytes())
            rec["jobs_cached"] = int(np.count_nonzero(last["gram"].fit_result.cached))
            if med.get("sklearn"):
                rec["sklearn_over_gram"], rec["sklearn_over_none"] = med["sklearn"] / med["gram"], med["sklearn"] / med["none"]
        job = [(np.arange(n), np.zeros(Z.shape[1]), np.ones(Z.shape[1]), 1.0)]
        rec["gram_pass_s"] = gram_pass(lambda **kw: aT.svc_fit_proba(Z, y.astype(np.int32), job, kernel=kernel, seeds=3, **kw))
        rec["chunks"], rec["peak_cache_bytes"], rec["groups_not_cached"] = layout([n], budget)
        t = int(np.argmax(fit.iterations[:, 0]))
        task = (fit.rows[t], fit.signs[t], np.zeros(Z.shape[1]), np.ones(Z.shape[1]), 1.0, None)
        rec["iteration_us_one_task_alone"] = iteration_us(aT, Z, task, kernel, modes)
        record("train_svm_device_" + kind, rec)

    # (c) silence_removal of one clip
    clip = base_clip(77)
    for name, repeat in (("20 s", 1), ("3 min", 9)):
        x = np.tile(clip, repeat)
        st, _ = stf.feature_extraction(x, FS, 0.05 * FS, 0.05 * FS)
        quiet, loud = aS._energy_extremes(st)
        rows = int(quiet.shape[1] + loud.shape[1])
        fns = {m: (lambda m=m: aS.silence_removal(x, FS, 0.05, 0.05, svm_fit="device", **cache[m])) for m in modes}
        if sklearn is not None:
            fns["sklearn"] = lambda: aS.silence_removal(x, FS, 0.05, 0.05)
        with one_core():
            med, every, last = alternate(fns, args.repeats)
        rec = {"seconds": len(x) / FS, "svm_rows": rows, "sklearn_s": med.get("sklearn")}
        rec.update({m + "_s": med[m] for m in modes})
        rec.update({k + "_s_all": v for k, v in every.items()})
        if not args.parent:
            rec["same_segments"] = last["gram"] == last["none"]
        F = np.vstack([quiet.T, loud.T])
        labels = np.append(np.zeros(quiet.shape[1]), np.ones(loud.shape[1])).astype(np.int32)
        mean, scale = F.mean(axis=0), np.sqrt(F.var(axis=0))
        scale[scale < 10 * np.finfo(np.float64).eps] = 1.0
        job = [(np.arange(rows), mean, scale, 1.0)]
        fit_call = lambda **kw: aT.svc_fit_proba(F, labels, job, seeds=7, **kw)      # noqa: E731
        fit_med, _, fit_last = alternate({m: (lambda m=m: fit_call(**cache[m])) for m in modes}, args.repeats)
        rec["fit_alone_s"] = fit_med
        rec["fit_iterations"] = fit_last["none"].iterations[0].tolist()
        rec["gram_pass_s"] = gram_pass(fit_call)
        rec["chunks"], rec["peak_cache_bytes"], rec["groups_not_cached"] = layout([rows], budget)
        task = (np.arange(rows), np.where(labels == 0, 1.0, -1.0), mean, scale, 1.0, None)
        rec["iteration_us_one_task_alone"] = iteration_us(aT, F, task, "linear", modes)
        record("silence_removal_" + name.replace(" ", "_"), rec)

    # (d) silence_removal_batch
    bases = [base_clip(k) for k in range(8)]
    sets = {"200x20_s": [bases[i % 8] for i in range(args.short)],
            "50x3_min": [np.concatenate([bases[(i + j) % 8] for j in range(9)]) for i in range(args.long)]}
    for name, clips in sets.items():
        fns = {m: (lambda m=m: aS.silence_removal_batch(clips, FS, 0.05, 0.05, return_details=True, **cache[m])) for m in modes}
        med, every, last = alternate(fns, args.repeats)
        details = last["none"][1]
        rows = [len(d["alpha_y"]) for d in details]
        rec = {"clips": len(clips), "seconds_per_clip": len(clips[0]) / FS, "svm_rows_min_max": [min(rows), max(rows)],
               "iterations_max": int(max(d["iterations"].max() for d in details))}
        rec.update({m + "_s": med[m] for m in modes})
        rec.update({k + "_s_all": v for k, v in every.items()})
        if not args.parent:
            rec["same_segments"] = last["gram"][0] == last["none"][0]
            rec["clips_cached"] = int(sum(d["cached"] for d in last["gram"][1]))
        # the fits' stage, the stream drained between the stages (no entry point of the batch takes max_iter: the Gram pass is inside)
        rec["fits_stage_ms"] = {}
        for m in modes:
            stage_ms = np.zeros(6)
            np.random.seed(5)
            kw = {} if m == "none" else dict(cache_bytes=budget)
            aS._silence_batch(clips, FS, 0.05, 0.05, 0.5, 0.5, lambda k: aS._batch_seeds(None, k), None, stage_ms=stage_ms, **kw)
            rec["fits_stage_ms"][m] = float(stage_ms[3])
        rec["gram_pass_s"] = None
        rec["chunks"], rec["peak_cache_bytes"], rec["groups_not_cached"] = layout(rows, budget)
        record("silence_batch_" + name, rec)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {m: v.get(m) for m in ("none_s", "gram_s", "sklearn_s", "gram_pass_s", "chunks", "peak_cache_bytes")}
                      for k, v in out["configurations"].items()}))


if __name__ == "__main__":
    main()
