#!/usr/bin/env python3
"""Measure the regression paths (not part of bench.py): the SVR bank kernel (kernels_svr.hpp) beside the SVC kernel of the same
work, the forest-regressor kind of the tree-ensemble kernels, and the file_regression drop-ins end to end.

    python scripts/bench_regress.py                   # GPU; writes profiles/bench_regress_n1_local.json and prints it
    python scripts/bench_regress.py --no-write

* SVR kernel, device-resident input, device time between two events on the library stream: (vector, model) pairs and
  (support vector, vector) pairs per second at three bank shapes -- 2 x (47 support vectors, 136 dims) on 36 000 windows (the
  arousal / valence models along a one-hour recording), 2 x (1 000, 136) on 36 000 windows, 100 x (42, 136) on 47 vectors
  (one parameter value of evaluate_regression on data/speechEmotion);
* the yardstick: svc_class_sums_kernel (+ its one-thread-per-window probability kernel) on a two-class model with the same
  support vectors and dims, in the same process -- the same kernel-value work with one coefficient row -- as (support vector,
  window) pairs per second, and the ratio of the two rates (a bank of ONE model, and the bank of two);
* forest regressors (seeded, 204 nodes per tree as the reference's trainer gives on knn_sm's rows) at 25 and 100 trees:
  windows per second;
* file_regression_signal host to host on a one-hour clip, file_regression_signals on 200 short clips against the loop of
  single calls, mid_term_regression_signal on the one-hour clip at a 0.1 s step;
* scikit-learn's per-vector predict loop on one core for scale (when scikit-learn is installed).
Rates are medians over --reps calls after one warm-up.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_classify import event_time, median_time, one_hour_clip  # noqa: E402

BANKS = {"2x47_on_36000": (2, 47, 36000), "2x1000_on_36000": (2, 1000, 36000), "100x42_on_47": (100, 42, 47)}
N_DIMS = 136


def seeded_svr(rng, n_sv, n_dims=N_DIMS):
    from pyaudioanalysis_amd import audioTrainTest
    return audioTrainTest.SvrArrays(rng.standard_normal((n_sv, n_dims)), rng.standard_normal((1, n_sv)), [rng.standard_normal()],
                                    1.0 / n_dims, "rbf")


def svc_of(svr):
    """A two-class probabilistic SVC with the SVR's support vectors (half per class) and coefficients."""
    from pyaudioanalysis_amd import audioTrainTest
    n = svr.support_vectors_.shape[0]
    return audioTrainTest.SvcArrays(svr.support_vectors_, [n // 2, n - n // 2], svr._dual_coef_, [0.1], [-1.0], [0.0], svr._gamma,
                                    "rbf", np.arange(2.0))


def kernels(args, out):
    from pyaudioanalysis_amd import _ffi, audioTrainTest
    lib = _ffi.lib()
    rng = np.random.default_rng(1)
    zeros, ones = np.zeros(N_DIMS), np.ones(N_DIMS)
    out["svr_kernel"] = {}
    for name, (n_models, n_sv, n_vec) in BANKS.items():
        models = [seeded_svr(rng, n_sv) for _ in range(n_models)]
        bufs = [_ffi.DeviceBuffer.from_host(rng.standard_normal((N_DIMS, n_vec))), _ffi.DeviceBuffer(8 * n_models * n_vec),
                _ffi.DeviceBuffer.from_host(np.concatenate([zeros, ones])), _ffi.DeviceBuffer(max(8, 4 * n_vec)), _ffi.DeviceBuffer(16 * n_vec)]
        d_x, d_out, d_stats, d_idx, d_proba = bufs
        row = {"models": n_models, "support_vectors_per_model": n_sv, "vectors": n_vec, "dims": N_DIMS}
        for label, members in (("bank", models), ("one_model", models[:1])):
            bank = audioTrainTest.SvrBank(members, zeros, ones)
            t = event_time(lambda: bank.predict_device(d_x, n_vec, n_vec, d_out), args.reps)
            row[label + "_s"] = t
            row[label + "_vector_model_pairs_per_s"] = len(members) * n_vec / t
            row[label + "_sv_vector_pairs_per_s"] = len(members) * n_sv * n_vec / t
        svc = audioTrainTest.SvcModel(svc_of(models[0]))
        t = event_time(lambda: _ffi.check(lib.paa_svc_dev_predict_f64(
            svc.handle, d_x.ptr, N_DIMS, n_vec, n_vec, d_stats.ptr, ctypes.c_void_p(d_stats.ptr.value + 8 * N_DIMS), d_idx.ptr,
            d_proba.ptr)), args.reps)
        row["svc_two_class_s"] = t
        row["svc_sv_window_pairs_per_s"] = n_sv * n_vec / t
        row["one_model_over_svc"] = row["one_model_sv_vector_pairs_per_s"] / row["svc_sv_window_pairs_per_s"]
        row["bank_over_svc"] = row["bank_sv_vector_pairs_per_s"] / row["svc_sv_window_pairs_per_s"]
        for b in bufs:
            b.free()
        out["svr_kernel"][name] = row
        print(name, row, file=sys.stderr)


def forests(args, out):
    import forest_ref
    from pyaudioanalysis_amd import _ffi, audioTrainTest
    rng = np.random.default_rng(2)
    out["forest_regressor_windows_per_s"] = {}
    n = args.windows
    zeros, ones = np.zeros(N_DIMS), np.ones(N_DIMS)
    made = {}
    for trees in (25, 100):
        a = forest_ref.synthetic_forest("averaged", trees, (143, 265), 23, 2, N_DIMS, 9)
        reg = audioTrainTest.ForestArrays("regressor", a.node_offsets, a.children_left, a.children_right, a.feature, a.threshold,
                                          a.missing_go_to_left, a.value[:, 0], None, N_DIMS)
        m = audioTrainTest.forest_model(reg)
        d_x = _ffi.DeviceBuffer.from_host(rng.standard_normal((N_DIMS, n)))
        t = median_time(lambda: m.predict_device(d_x, n, n, zeros, ones), args.reps)
        d_x.free()
        out["forest_regressor_windows_per_s"]["rf%d" % trees] = n / t
        made[trees] = reg
    out["forest_windows_per_call"] = n
    return made


def end_to_end(args, out, forest25):
    from pyaudioanalysis_amd import audioSegmentation, audioTrainTest
    rng = np.random.default_rng(3)
    models = [seeded_svr(rng, 47), seeded_svr(rng, 47)]
    means, stds = rng.standard_normal((2, N_DIMS)) * 0.1, rng.uniform(0.5, 2.0, (2, N_DIMS))
    clip = one_hour_clip()
    reps = max(1, args.reps // 4)
    windows = (1.0, 1.0, 0.05, 0.05, False)
    out["one_hour_file_regression_signal_s"] = {
        "svm_rbf": median_time(lambda: audioTrainTest.file_regression_signal(clip, 16000, models, means, stds, *windows, "svm_rbf"), reps),
        "randomforest": median_time(lambda: audioTrainTest.file_regression_signal(clip, 16000, [forest25, forest25], means, stds,
                                                                                 *windows, "randomforest"), reps)}
    out["one_hour_mid_term_regression_step0.1_s"] = {
        "svm_rbf": median_time(lambda: audioSegmentation.mid_term_regression_signal(clip, 16000, models, means, stds, "svm_rbf", 1.0, 0.1,
                                                                                   0.05, 0.05), reps),
        "randomforest": median_time(lambda: audioSegmentation.mid_term_regression_signal(clip, 16000, [forest25, forest25], means, stds,
                                                                                        "randomforest", 1.0, 0.1, 0.05, 0.05), reps)}
    shorts = [clip[i * 48000:i * 48000 + int(rng.integers(24000, 48000))] for i in range(200)]
    t_batch = median_time(lambda: audioTrainTest.file_regression_signals(shorts, 16000, models, means, stds, *windows, "svm_rbf"), reps)
    t_loop = median_time(lambda: [audioTrainTest.file_regression_signal(s, 16000, models, means, stds, *windows, "svm_rbf")
                                  for s in shorts], 1)
    out["short_clips_200"] = {"batch_s": t_batch, "loop_of_single_calls_s": t_loop}


def sklearn_loop(args, out):
    try:
        from sklearn.svm import SVR
    except ImportError:
        return
    rng = np.random.default_rng(4)
    Xtr = rng.standard_normal((47, N_DIMS))
    model = SVR(kernel="rbf", C=1.0).fit(Xtr, rng.standard_normal(47))
    X = rng.standard_normal((args.loop_vectors, N_DIMS))
    t0 = time.perf_counter()
    for v in X:                      # audioTrainTest.regression_wrapper (:109-111), once per vector
        model.predict(v.reshape(1, -1))[0]
    out["sklearn_per_vector_loop_vectors_per_s"] = {"svr_47x136": args.loop_vectors / (time.perf_counter() - t0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--loop-vectors", type=int, default=2000)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    from pyaudioanalysis_amd import _ffi
    _ffi.init(0)
    out = {"what": "regression paths on one MI355X (scripts/bench_regress.py)", "reps": args.reps}
    kernels(args, out)
    made = forests(args, out)
    end_to_end(args, out, made[25])
    sklearn_loop(args, out)
    line = json.dumps(out)
    if not args.no_write:
        with open(os.path.join(ROOT, "profiles", "bench_regress_n1_local.json"), "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(line)


if __name__ == "__main__":
    main()
