#!/usr/bin/env python3
"""Times the probabilistic SVM fit on the GPU (kernels_smo.hpp, kernels_platt.hpp) against scikit-learn's SVC(probability=True) on
this host's CPU, one thread.  Writes profiles/bench_platt_n1_local.json.  Runs on the GPU.

(a) audioSegmentation.silence_removal on clips of 20 s, 3 min and 30 min at 16 kHz with a 50 ms window and step (a 20 s synthetic
    clip with digital silence between bursts, repeated): host-to-host time of svm_fit="device" and of svm_fit="sklearn", the DEVICE
    time between two events on the library's stream around the device-mode call, and the rows of the onset SVM's one pair.
(b) audioTrainTest.train_svm_device on 5 000 x 136 with 8 classes (28 pairs, at most 168 tasks), linear and RBF at C = 1:
    host-to-host and device time of the call, the tasks' iteration counts, and scikit-learn's fit of the same data.
Beside both: the device time of one platt_sigmoid call on the held-out decision values of that fit (its copies included, so an
upper bound) and its share of the fit's device time.  A record, not a gate; the scikit-learn figures are null where it cannot be
imported.

Every host-to-host comparison alternates the two modes for --repeats rounds after a warm-up and reports the median beside every
single time; the silence_removal windows are milliseconds long, so read them as latencies, not rates.

    python scripts/bench_platt.py [--samples 5000] [--repeats 5] [--no-sklearn] [--out FILE]
"""
import argparse
import contextlib
import ctypes
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

FS = 16000
CLIPS = (("20 s", 1), ("3 min", 9), ("30 min", 90))


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


def alternate(rec, fns, repeats):
    """Times the calls of fns {name: fn} alternately, `repeats` rounds (every call ends in a device synchronise or runs on the CPU):
    rec[name] = the median, rec[name + "_all"] = every time.  Returns the last return value of each."""
    times, last = {k: [] for k in fns}, {}
    for _ in range(repeats):
        for k, fn in fns.items():
            np.random.seed(5)
            t, last[k] = host_time(fn)
            times[k].append(t)
    for k, v in times.items():
        rec[k], rec[k + "_all"] = float(np.median(v)), v
    return last


def base_clip():
    from synth import synth_clip
    x = synth_clip(777, 20 * FS).copy()
    rng = np.random.default_rng(3)
    for _ in range(8):                                  # digital silence between bursts
        a = int(rng.integers(0, 19 * FS))
        x[a:a + int(rng.integers(FS // 4, FS))] = 0
    return x


def sigmoid_share(aT, fit, fit_device_s):
    """device time of one platt_sigmoid call on the fit's held-out values, and its share of the fit's device time"""
    dec = np.concatenate(fit.cv_dec)
    signs = np.concatenate(fit.signs)
    off = np.concatenate([[0], np.cumsum([len(r) for r in fit.rows])])
    aT.platt_sigmoid(dec, signs, off)
    s, res = event_time(lambda: aT.platt_sigmoid(dec, signs, off))
    return {"sigmoid_call_device_s": s, "sigmoid_share_of_fit": s / fit_device_s, "sigmoid_iterations_max": int(res.iterations.max()),
            "sigmoid_problems": len(fit.rows), "sigmoid_values": int(off[-1])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--repeats", type=int, default=5, help="rounds of every host-to-host comparison; the median is reported")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_platt_n1_local.json"))
    args = ap.parse_args()
    import train_ref
    from pyaudioanalysis_amd import ShortTermFeatures as stf, _ffi, audioSegmentation as aS, audioTrainTest as aT
    if _ffi.device_count() < 1:
        raise SystemExit("bench_platt.py needs a HIP device")
    _ffi.init(0)
    try:
        if args.no_sklearn:
            raise ImportError
        import sklearn.svm
        from threadpoolctl import threadpool_limits
    except ImportError:
        sklearn = None
    out = {"silence_removal": {}, "train_svm_device": {}}
    warnings.simplefilter("ignore")

    # (a) silence_removal
    clip = base_clip()
    aS.silence_removal(clip, FS, 0.05, 0.05, svm_fit="device", random_state=1)          # warm-up: library, plans, lane scratch
    for name, repeat in CLIPS:
        x = np.tile(clip, repeat)
        rec = {"seconds": len(x) / FS}
        st, _ = stf.feature_extraction(x, FS, 0.05 * FS, 0.05 * FS)
        quiet, loud = aS._energy_extremes(st)
        rec["frames"], rec["svm_rows"] = int(st.shape[1]), int(quiet.shape[1] + loud.shape[1])
        try:
            np.random.seed(5)
            rec["device_mode_device_s"], segs = event_time(lambda: aS.silence_removal(x, FS, 0.05, 0.05, svm_fit="device"))
            device_ok = True
            feats = np.vstack([quiet.T, loud.T])
            labels = np.append(np.zeros(quiet.shape[1]), np.ones(loud.shape[1]))
            mean, scale = feats.mean(axis=0), np.sqrt(feats.var(axis=0))
            scale[scale < 10 * np.finfo(np.float64).eps] = 1.0
            job = [(np.arange(len(labels)), mean, scale, 1.0)]
            rec["fit_device_s"], fit = event_time(lambda: aT.svc_fit_proba(feats, labels, job, seeds=7, return_cv=True))
            rec["fit_tasks"], rec["fit_iterations"] = int(np.count_nonzero(fit.status)), fit.iterations[0].tolist()
            rec["fit_solver_launches"] = fit.n_launches
            rec.update(sigmoid_share(aT, fit, rec["fit_device_s"]))
        except NotImplementedError as exc:              # the onset SVM's pair is above the solver's row limit
            rec["device_mode_refused"] = str(exc)
            device_ok = False
        rec["sklearn_mode_host_s"] = None
        fns = {}
        if device_ok:
            fns["device_mode_host_s"] = lambda: aS.silence_removal(x, FS, 0.05, 0.05, svm_fit="device")
        if sklearn is not None:
            fns["sklearn_mode_host_s"] = lambda: aS.silence_removal(x, FS, 0.05, 0.05)
        with (threadpool_limits(limits=1) if sklearn is not None else contextlib.nullcontext()):
            last = alternate(rec, fns, args.repeats)
        rec["segments"] = {k: len(v) for k, v in last.items()}
        print("silence_removal %s: %s" % (name, json.dumps(rec)), file=sys.stderr, flush=True)
        out["silence_removal"][name] = rec

    # (b) train_svm_device
    feats = train_ref.bench_features(args.samples)
    X, y = train_ref.features_to_matrix(feats)
    Z = (X - X.mean(axis=0)) / X.std(axis=0)
    out["samples"], out["dims"], out["classes"] = int(X.shape[0]), int(X.shape[1]), len(feats)
    aT.train_svm_device(Z[::10], y[::10], 1.0, random_state=1)                          # warm-up
    for kind, kernel in (("svm", "linear"), ("svm_rbf", "rbf")):
        rec = {}
        rec["device_s"], model = event_time(lambda: aT.train_svm_device(Z, y, 1.0, kernel, random_state=3))
        fns = {"host_s": lambda: aT.train_svm_device(Z, y, 1.0, kernel, random_state=3)}
        if sklearn is not None:
            fns["sklearn_host_s"] = lambda: sklearn.svm.SVC(C=1.0, kernel=kernel, probability=True, gamma="auto", random_state=3).fit(Z, y)
        with (threadpool_limits(limits=1) if sklearn is not None else contextlib.nullcontext()):
            last = alternate(rec, fns, args.repeats)
        model = last["host_s"]
        fit = model.fit_result
        rec.update({"pairs": len(fit.rows), "tasks": int(np.count_nonzero(fit.status)), "iterations_total": int(fit.iterations.sum()),
                    "iterations_max": int(fit.iterations.max()), "solver_launches": fit.n_launches,
                    "not_converged": int(np.count_nonzero(fit.status == aT.SMO_NOT_CONVERGED)), "support_vectors": int(len(model.support_))})
        job = [(np.arange(len(y)), np.zeros(Z.shape[1]), np.ones(Z.shape[1]), 1.0)]
        fit = aT.svc_fit_proba(Z, y.astype(np.int32), job, kernel=kernel, seeds=model.random_seed, return_cv=True)
        rec.update(sigmoid_share(aT, fit, rec["device_s"]))
        rec.setdefault("sklearn_host_s", None)
        if sklearn is not None:
            sk = last["sklearn_host_s"]
            rec["probA_distance_to_sklearn"] = float(np.max(np.abs(model.probA_ - sk.probA_)))
            rec["probB_distance_to_sklearn"] = float(np.max(np.abs(model.probB_ - sk.probB_)))
            rec["proba_distance_to_sklearn"] = float(np.max(np.abs(aT.svm_predict(model, Z[::25].T, np.zeros(Z.shape[1]), np.ones(Z.shape[1]))[1]
                                                                   - sk.predict_proba(Z[::25]))))
        print("train_svm_device %s: %s" % (kind, json.dumps(rec)), file=sys.stderr, flush=True)
        out["train_svm_device"][kind] = rec
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
