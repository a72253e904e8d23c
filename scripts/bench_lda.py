#!/usr/bin/env python3
"""Times the LDA step of GPU speaker diarization (kernels_lda.hpp) on the one-hour shape: 72 000 windows x 148 dims in 720
classes of 100 windows, lda_dim 35, on a seeded synthetic matrix.  Writes profiles/bench_lda_n1_local.json.  Runs on the GPU.

Per entry point (class statistics, within-class Gram matrix, projection) the median DEVICE time between two events on the
library's stream around the call -- the kernels plus the call's small copies (run offsets, class means, the 148 x 148
result); the host eigen step (numpy.linalg.eigh twice) by the host clock; fit + transform end to end and
speaker_diarization_lda_signal host to host by the host clock around calls that end in a device synchronise.  The Gram
kernel's FP64 rate counts the multiply-adds of the upper-triangle 32 x 32 blocks it computes and is set against the data
sheet's FP64 vector peak (the matrix and the vector unit issue FP64 at the same rate on this part).  Beside them, where
scikit-learn can be imported, its LinearDiscriminantAnalysis.fit_transform of the same matrix on one core: a record, not
a gate.

    python scripts/bench_lda.py [--reps 9] [--windows 72000]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FP64_VECTOR_PEAK = 78.6e12        # MI355X data sheet, FP64 vector, FMA = 2 flop


def median_time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def event_time(fn, reps):
    """Median device time in seconds between two events on the library stream around fn() (one warm-up call first)."""
    from pyaudioanalysis_amd import _ffi
    lib = _ffi.lib()
    fn()
    ts = []
    for _ in range(reps):
        ms = ctypes.c_float()
        _ffi.check(lib.paa_timer_start())
        fn()
        _ffi.check(lib.paa_timer_stop(ctypes.byref(ms)))
        ts.append(ms.value * 1e-3)
    return float(np.median(ts))


def planted(n, d, run, speakers, seed):
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((speakers, d)) * 1.5
    who = np.repeat(rng.integers(speakers, size=(n + run - 1) // run), run)[:n]
    X = means[who] + rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, d)
    return np.ascontiguousarray(X), (np.arange(n) // run).astype(np.int64)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--windows", type=int, default=72000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_lda_n1_local.json"))
    args = ap.parse_args()
    from pyaudioanalysis_amd import _ffi, audioSegmentation as aS
    if _ffi.device_count() < 1:
        raise SystemExit("bench_lda.py needs a HIP device")
    _ffi.init(0)
    lib = _ffi.lib()
    n, D, run, dim = args.windows, 148, 100, 35
    X, labels = planted(n, D, run, 6, 23)
    off = aS._lda_runs(labels, n)
    C = off.shape[0] - 1
    out = {"windows": n, "dims": D, "classes": C, "lda_dim": dim, "reps": args.reps}
    d_x = _ffi.DeviceBuffer.from_host(np.ascontiguousarray(X.T))
    means, std, G = np.empty((C, D)), np.empty(D), np.empty((D, D))
    fac = 1.0 / (n - C)
    stats = lambda: _ffi.check(lib.paa_lda_dev_class_stats_f64(d_x.ptr, D, n, n, _ffi.as_i64p(off), C, _ffi.as_f64p(means), _ffi.as_f64p(std)))
    gram = lambda: _ffi.check(lib.paa_lda_dev_within_gram_f64(d_x.ptr, D, n, n, _ffi.as_i64p(off), C, _ffi.as_f64p(means), _ffi.as_f64p(std),
                                                            fac, _ffi.as_f64p(G)))
    out["class_stats_call_s"] = event_time(stats, args.reps)
    out["within_gram_call_s"] = event_time(gram, args.reps)
    blocks = (D + 31) // 32
    flop = 2.0 * (blocks * (blocks + 1) // 2) * 32 * 32 * n
    out["within_gram_fp64_flop"] = flop
    out["within_gram_call_fp64_share_of_vector_peak"] = flop / out["within_gram_call_s"] / FP64_VECTOR_PEAK
    out["within_gram_algorithmic_bytes"] = n * D * 8
    tiles = (D + 63) // 64
    out["within_gram_panel_bytes_requested"] = (tiles + tiles * (tiles - 1)) * 64 * n * 8      # served by L2 / HBM: not measured
    out["within_gram_partial_bytes_written"] = ((n + 1023) // 1024) * D * D * 8
    model = aS.lda_fit_device(d_x, D, n, n, labels, dim)
    d_y = _ffi.DeviceBuffer(dim * n * 8)
    proj = lambda: aS.lda_transform_device(model, d_x, D, n, n, d_y, n)
    out["project_call_s"] = event_time(proj, args.reps)
    out["project_fp64_flop"] = 2.0 * n * D * dim
    d_y.free()

    def eigen():
        S, V = aS._eigh_desc(G)
        W = np.random.default_rng(0).standard_normal((C, model["rank"]))
        aS._eigh_desc(W.T @ W)
    out["host_eigen_s"] = median_time(eigen, args.reps)

    def fit_transform():
        m = aS.lda_fit_device(d_x, D, n, n, labels, dim)
        aS.lda_transform_device(m, d_x, D, n, n)[0].free()
    out["fit_transform_device_resident_s"] = median_time(fit_transform, args.reps)
    out["rank"], out["rank2"] = model["rank"], model["rank2"]
    d_x.free()
    out["fit_transform_host_to_host_s"] = median_time(lambda: aS.lda_fit_transform(X, labels, dim), max(1, args.reps // 3))
    try:
        from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
        from threadpoolctl import threadpool_limits
        with threadpool_limits(limits=1):
            t0 = time.perf_counter()
            ref = LinearDiscriminantAnalysis(n_components=dim).fit_transform(X, labels)
            out["sklearn_fit_transform_one_core_s"] = time.perf_counter() - t0
        import lda_ref
        got = aS.lda_fit_transform(X, labels, dim)
        _, flips, _ = lda_ref.sign_fix(LinearDiscriminantAnalysis(n_components=dim).fit(X, labels).scalings_[:, :dim])
        out["max_err_vs_sklearn"] = float(np.max(np.abs(got - ref * flips)) / max(np.max(np.abs(ref)), 1.0))
    except ImportError as exc:
        out["sklearn_fit_transform_one_core_s"] = "not measured: %s" % exc
    # the whole branch on one hour of audio, host to host, with seeded SVMs of the shipped shapes
    from synth import synth_clip
    from lda_ref import synthetic_speaker_models as synthetic_models
    fs = 16000
    clip = np.concatenate([synth_clip(s, 10 * fs) for s in (1, 2, 3, 4, 5, 6)] * 60)
    models = synthetic_models()
    run_signal = lambda: aS.speaker_diarization_lda_signal(clip, fs, 0, 1.0, 0.1, 0.1, dim, models=models, random_state=3)
    out["signal_seconds_of_audio"] = len(clip) / fs
    out["speaker_diarization_lda_signal_host_s"] = median_time(run_signal, 2)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
