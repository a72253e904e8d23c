#!/usr/bin/env python3
"""Measure the SVM, kNN and tree-ensemble classification paths (not part of bench.py).

    python scripts/bench_classify.py --diar                # GPU: speaker diarization (k-means sweep, silhouettes; DESIGN K11)
    python scripts/bench_classify.py --hmm                 # GPU: the HMM segmenter (emission + Viterbi)
    python scripts/bench_classify.py                       # GPU: SVC and kNN kernel rates per shipped model, 1 h clip end
                                                           # to end
    python scripts/bench_classify.py --forest              # GPU: tree-ensemble rates per model shape, 1 h clip end to end
    python scripts/bench_classify.py --train               # GPU: evaluate_classifier("knn"), the split sweep in one launch against
                                                           # the per-split loop of paa_knn_create / predict / destroy (DESIGN K14)
    python scripts/bench_classify.py --reference-loop DIR  # host: the reference's per-window loops (SVM: scikit-learn;
                                                           # kNN: NumPy + SciPy) (DIR = pyAudioAnalysis/data/models)

The models: svm_rbf_sm, svm_rbf_speaker_male_female and svm_rbf_musical_genre_6 from the svc_* goldens (tests/golden, arrays
only); svm_rbf_speaker_10 and svm_rbf_movie8class, whose arrays are too large for a golden file, as seeded models of exactly their
shape (tests/svc_libsvm.synthetic_model: same classes, support vectors per class and dims -- the work per window is the same).
The kNN models: knn_musical_genre_6 from the knn_genre6_files golden (the real model); knn_sm, knn_speaker_male_female,
knn_speaker_10 and knn_movie8class as seeded models of exactly their shape (training rows x dims, k, classes: the work per
window is the same).  The kNN entry also gives the FP64 work per window, 3 n_train n_dims (a subtraction, a multiply and an
add per training row and dimension).
The tree ensembles (--forest): seeded models (tests/forest_ref.synthetic_forest) of the shapes that the reference's own
trainers give on the shipped kNN models' training rows (trees, nodes per tree, depth, classes, dims), plus
RandomForest-500 at knn_movie8class's shape and a 64-class x 256-dim forest.
All use 1 s / 1 s mid-term and 50 ms / 50 ms short-term windows, as the shipped models do.  Rates are medians over --reps
calls after one warm-up.  Prints one JSON line.
"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svc_libsvm  # noqa: E402

GOLDEN_MODELS = {"svm_rbf_sm": "svc_sm_speech_music", "svm_rbf_speaker_male_female": "svc_malefemale_diarization",
                 "svm_rbf_musical_genre_6": "svc_genre6_files"}
SHAPED_MODELS = {"svm_rbf_speaker_10": svc_libsvm.SPEAKER_10_N_SUPPORT, "svm_rbf_movie8class": svc_libsvm.MOVIE8CLASS_N_SUPPORT}
MODELS = ["svm_rbf_sm", "svm_rbf_speaker_male_female", "svm_rbf_speaker_10", "svm_rbf_movie8class", "svm_rbf_musical_genre_6"]
# kNN: (training rows, dims, k, classes) of the shipped models; knn_musical_genre_6 is the real one (golden)
KNN_SHAPES = {"knn_sm": (2422, 136, 5, 2), "knn_speaker_male_female": (1498, 136, 1, 2), "knn_speaker_10": (1294, 136, 9, 10),
              "knn_movie8class": (3040, 136, 9, 8), "knn_musical_genre_6": (581, 138, 5, 6)}
KNN_GOLDEN = {"knn_musical_genre_6": "knn_genre6_files"}


def golden(name):
    with np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def median_time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def one_hour_clip(fs=16000, seconds=3600):
    rng = np.random.default_rng(5)
    t = np.arange(seconds * fs, dtype=np.float64) / fs
    x = 8000 * np.sin(2 * np.pi * 220 * t * (1 + 0.3 * np.sin(2 * np.pi * t / 97))) * (0.5 + 0.5 * np.sin(2 * np.pi * t / 13))
    x += rng.normal(0, 1500, t.shape[0]) * (np.sin(2 * np.pi * t / 41) > 0)
    return np.clip(x, -32768, 32767).astype(np.int16)


def gpu(args):
    from pyaudioanalysis_amd import MidTermFeatures, _ffi, audioSegmentation, audioTrainTest
    _ffi.init(0)
    out = {"kernel_windows_per_s": {}, "one_hour_s": {}}
    rng = np.random.default_rng(1)
    clip = one_hour_clip()
    mid, _, _ = MidTermFeatures.mid_feature_extraction(clip, 16000, 16000, 16000, 800, 800)
    clip_mean, clip_std = mid.mean(axis=1), np.where(mid.std(axis=1) > 0, mid.std(axis=1), 1.0)
    for model in MODELS:
        if model in GOLDEN_MODELS:
            g = golden(GOLDEN_MODELS[model])
            arrays = (g["sv"], g["n_support"], g["dual_coef"], -g["rho"], g["prob_a"], g["prob_b"], g["gamma"], str(g["kernel"]),
                      g["classes"])
            mean, std, beat = g["mean"], g["std"], "compute_beat" in g and bool(g["compute_beat"])
        else:
            m = svc_libsvm.synthetic_model(SHAPED_MODELS[model], 136, 3)
            arrays = (m["support_vectors"], m["n_support"], m["dual_coef"], -m["rho"], m["prob_a"], m["prob_b"], m["gamma"],
                      "rbf", np.arange(len(m["n_support"]), dtype=np.float64))
            mean, std, beat = clip_mean, clip_std, False
        svc = audioTrainTest.SvcModel(audioTrainTest.SvcArrays(*arrays))
        n_dims = svc.n_dims
        X = rng.standard_normal((n_dims, args.windows))
        d_x = _ffi.DeviceBuffer.from_host(X)
        zeros, ones = np.zeros(n_dims), np.ones(n_dims)
        t = median_time(lambda: svc.predict_device(d_x, args.windows, args.windows, zeros, ones), args.reps)
        out["kernel_windows_per_s"][model] = args.windows / t
        d_x.free()
        if not beat:           # mid_term_file_classification refuses beat models (audioSegmentation.py:566-570)
            t = median_time(lambda: audioSegmentation.mid_term_labels(clip, 16000, svc, mean, std, 1.0, 1.0, 0.05, 0.05),
                            max(1, args.reps // 4))
            out["one_hour_s"][model] = t
        print(model, {k: v.get(model) for k, v in out.items()}, file=sys.stderr)
    knn(args, out, clip, clip_mean, clip_std)
    out["windows_per_call"] = args.windows
    return out


def knn_seeded(n_train, n_dims, k, n_classes, seed=3):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, n_classes, n_train).astype(np.float64)
    labels[:n_classes] = np.arange(n_classes)
    return rng.standard_normal((n_train, n_dims)), labels, k


def knn(args, out, clip, clip_mean, clip_std):
    from pyaudioanalysis_amd import _ffi, audioSegmentation, audioTrainTest
    rng = np.random.default_rng(2)
    out.update({"knn_windows_per_s": {}, "knn_one_hour_s": {}, "knn_fp64_flop_per_window": {}})
    for model, (n_train, n_dims, k, n_classes) in KNN_SHAPES.items():
        if model in KNN_GOLDEN:
            g = golden(KNN_GOLDEN[model])
            clf = audioTrainTest.Knn(g["features"], g["labels"], int(g["neighbors"]))
            mean, std, beat = g["mean"], g["std"], bool(g["compute_beat"])
        else:
            clf = audioTrainTest.Knn(*knn_seeded(n_train, n_dims, k, n_classes))
            mean, std, beat = clip_mean, clip_std, False
        m = audioTrainTest.knn_model(clf)
        assert (m.n_dims, m.k, m.n_classes) == (n_dims, k, n_classes)
        d_x = _ffi.DeviceBuffer.from_host(rng.standard_normal((n_dims, args.windows)))
        zeros, ones = np.zeros(n_dims), np.ones(n_dims)
        t = median_time(lambda: m.predict_device(d_x, args.windows, args.windows, zeros, ones), args.reps)
        out["knn_windows_per_s"][model] = args.windows / t
        out["knn_fp64_flop_per_window"][model] = 3 * n_train * n_dims
        d_x.free()
        if not beat:           # mid_term_file_classification refuses beat models (audioSegmentation.py:566-570)
            t = median_time(lambda: audioSegmentation.mid_term_labels(clip, 16000, clf, mean, std, 1.0, 1.0, 0.05, 0.05, "knn"),
                            max(1, args.reps // 4))
            out["knn_one_hour_s"][model] = t
        print(model, {key: out[key].get(model) for key in ("knn_windows_per_s", "knn_one_hour_s")}, file=sys.stderr)


# name: (kind, trees or stages, mean nodes per tree, max depth, classes, dims)
FOREST_SHAPES = {"sm_rf25": ("averaged", 25, 204, 23, 2, 136), "sm_rf100": ("averaged", 100, 204, 23, 2, 136),
                 "sm_et25": ("averaged", 25, 603, 25, 2, 136), "sm_gb100": ("boosted", 100, 14, 3, 2, 136),
                 "movie8_rf25": ("averaged", 25, 1150, 27, 8, 136), "movie8_rf100": ("averaged", 100, 1150, 27, 8, 136),
                 "movie8_et25": ("averaged", 25, 2692, 33, 8, 136), "movie8_gb100": ("boosted", 100, 14, 3, 8, 136),
                 "movie8_rf500": ("averaged", 500, 1150, 27, 8, 136),
                 "genre6_rf100": ("averaged", 100, 157, 18, 6, 138), "genre6_gb100": ("boosted", 100, 14, 3, 6, 138),
                 "c64_d256_rf100": ("averaged", 100, 1000, 24, 64, 256)}


def forest(args):
    import forest_ref
    from pyaudioanalysis_amd import MidTermFeatures, _ffi, audioSegmentation, audioTrainTest
    _ffi.init(0)
    out = {"forest_windows_per_s": {}, "forest_one_hour_s": {}, "forest_nodes": {}}
    rng = np.random.default_rng(2)
    clip = one_hour_clip()
    mid, _, _ = MidTermFeatures.mid_feature_extraction(clip, 16000, 16000, 16000, 800, 800)
    clip_mean, clip_std = mid.mean(axis=1), np.where(mid.std(axis=1) > 0, mid.std(axis=1), 1.0)
    for name, (kind, trees, nodes, depth, n_classes, n_dims) in FOREST_SHAPES.items():
        a = forest_ref.synthetic_forest(kind, trees, (int(nodes * 0.7), int(nodes * 1.3)), depth, n_classes, n_dims, 9)
        m = audioTrainTest.forest_model(a)
        out["forest_nodes"][name] = int(a.threshold.shape[0])
        d_x = _ffi.DeviceBuffer.from_host(rng.standard_normal((n_dims, args.windows)))
        zeros, ones = np.zeros(n_dims), np.ones(n_dims)
        t = median_time(lambda: m.predict_device(d_x, args.windows, args.windows, zeros, ones), args.reps)
        out["forest_windows_per_s"][name] = args.windows / t
        d_x.free()
        if n_dims == 136:
            model_type = "gradientboosting" if kind == "boosted" else "randomforest"
            t = median_time(lambda: audioSegmentation.mid_term_labels(clip, 16000, a, clip_mean, clip_std, 1.0, 1.0, 0.05, 0.05,
                                                                      model_type), max(1, args.reps // 4))
            out["forest_one_hour_s"][name] = t
            if name == "movie8_rf100":       # the 0.1 s mid-term step: 36 000 windows
                t = median_time(lambda: audioSegmentation.mid_term_labels(clip, 16000, a, clip_mean, clip_std, 1.0, 0.1, 0.05,
                                                                          0.05, model_type), max(1, args.reps // 4))
                out["forest_one_hour_s"][name + "_step0.1"] = t
        print(name, {k: v.get(name) for k, v in out.items()}, file=sys.stderr)
    out["windows_per_call"] = args.windows
    return out


def hmm(args):
    """Emission + Viterbi rates (device-resident windows), the block decode against the one-wave serial decode of the same
    sequence, the ragged batch, hmm_segmentation's labels of the 1-hour clip beside mid_term_labels with svm_rbf_sm, and the
    NumPy restatement on one core for scale.  Runs on the GPU."""
    import hmm_ref
    from pyaudioanalysis_amd import _ffi, audioSegmentation, audioTrainTest
    _ffi.init(0)
    out = {"hmm_windows_per_s": {}, "hmm_block_s": {}, "hmm_one_wave_s": {}, "hmm_emission_s": {}, "hmm_one_hour_s": {},
           "hmm_numpy_windows_per_s": {}}
    T, D = 36000, 136
    for K in (2, 4, 8, 32):
        model = hmm_ref.synthetic_model(K, D, 40 + K)
        X = hmm_ref.synthetic_sequence(model, T, 50 + K)
        h = audioSegmentation.GaussianHmm(*model)
        d_x = _ffi.DeviceBuffer.from_host(np.ascontiguousarray(X.T))
        t_block = median_time(lambda: h.predict_device(d_x, T, T), args.reps)
        t_wave = median_time(lambda: h.predict_device(d_x, T, T, None, T), max(2, args.reps // 2))
        t_emit = median_time(lambda: h.log_likelihood_device(d_x, T, T), args.reps)
        _, a = h.predict_device(d_x, T, T)
        _, b = h.predict_device(d_x, T, T, None, T)
        out["hmm_windows_per_s"][K] = T / t_block
        out["hmm_block_s"][K], out["hmm_one_wave_s"][K], out["hmm_emission_s"][K] = t_block, t_wave, t_emit
        out.setdefault("hmm_block_equals_one_wave", {})[K] = bool(np.array_equal(a, b))
        d_x.free()
        if K in (2, 8):
            t0 = time.perf_counter()
            hmm_ref.decode(*model, X[:6000])
            out["hmm_numpy_windows_per_s"][K] = 6000 / (time.perf_counter() - t0)
        print("hmm K", K, {k: v.get(K) for k, v in out.items() if isinstance(v, dict)}, file=sys.stderr)
    out["hmm_emission_bytes"] = T * D * 8
    # ragged batch: 1 000 sequences of 1 .. 600 windows, K = 4, D = 8
    model = hmm_ref.synthetic_model(4, 8, 31)
    lengths = np.random.default_rng(31).integers(1, 601, 1000)
    X = hmm_ref.synthetic_sequence(model, int(lengths.sum()), 1031)
    h = audioSegmentation.GaussianHmm(*model)
    d_x = _ffi.DeviceBuffer.from_host(np.ascontiguousarray(X.T))
    offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    t = median_time(lambda: h.predict_device(d_x, X.shape[0], X.shape[0], offsets), args.reps)
    out["hmm_ragged_windows_per_s"] = X.shape[0] / t
    d_x.free()
    # one hour, host to host: the shipped model's shape (K = 2) beside the SVM path at the same steps
    clip = one_hour_clip()
    model = hmm_ref.synthetic_model(2, 136, 7)
    h = audioSegmentation.GaussianHmm(*model)
    g = golden(GOLDEN_MODELS["svm_rbf_sm"])
    svc = audioTrainTest.SvcModel(audioTrainTest.SvcArrays(g["sv"], g["n_support"], g["dual_coef"], -g["rho"], g["prob_a"],
                                                           g["prob_b"], g["gamma"], str(g["kernel"]), g["classes"]))
    for step in (1.0, 0.1):
        out["hmm_one_hour_s"]["hmm_step%g" % step] = median_time(
            lambda: audioSegmentation.hmm_labels(clip, 16000, h, 1.0, step), max(1, args.reps // 4))
        out["hmm_one_hour_s"]["svm_rbf_sm_step%g" % step] = median_time(
            lambda: audioSegmentation.mid_term_labels(clip, 16000, svc, g["mean"], g["std"], 1.0, step, 0.05, 0.05),
            max(1, args.reps // 4))
    return out


def event_time(fn, reps):
    """Median device time in seconds between two events on the library stream around fn() (one warm-up call first)."""
    import ctypes
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


def planted_speakers(n, d, speakers, seed, dwell=40):
    """(M [d][n], speaker of every window): Gaussian speakers that change about every `dwell` windows."""
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((speakers, d)) * 1.5
    path = np.empty(n, dtype=np.int64)
    s = 0
    for t in range(n):
        if t % dwell == 0:
            s = int(rng.integers(speakers))
        path[t] = s
    return np.ascontiguousarray((means[path] + rng.standard_normal((n, d))).T), path


FP64_VECTOR_PEAK = 78.6e12        # MI355X data sheet, FP64 vector, FMA = 2 flop


def diar(args):
    """Speaker diarization at N = 36 000 windows x 148 dims (one hour at the default 0.1 s step): the cluster-pair kernel alone
    (all k = 2..9 in one pass, and one k), the k = 2..9 sweep (steps 3-6, device-resident input), diarize_features host to
    host, speaker_diarization_signal on the 1-hour clip with seeded SVMs of the shipped shapes, and the reference-side step
    6 (cdist blocks) on one core at a smaller N.  Runs on the GPU."""
    import ctypes
    from scipy.spatial import distance
    from pyaudioanalysis_amd import _ffi, audioSegmentation, audioTrainTest
    _ffi.init(0)
    lib = _ffi.lib()
    N, D = args.diar_windows, 148
    out = {"diar_windows": N, "diar_dims": D}
    M, path = planted_speakers(N, D, 6, 17)
    ks = np.arange(2, 10, dtype=np.int32)
    labels = np.stack([path % k for k in ks]).astype(np.int32)
    d_m, d_l = _ffi.DeviceBuffer.from_host(M), _ffi.DeviceBuffer.from_host(labels)
    S = np.empty((len(ks), 32, 32))

    def pair(nk):
        _ffi.check(lib.paa_diar_dev_pair_sums_f64(d_m.ptr, D, N, N, ctypes.c_void_p(d_l.ptr.value + (len(ks) - nk) * N * 4),
                                                  ks[len(ks) - nk:].ctypes.data_as(_ffi.c_i32p), nk, _ffi.as_f64p(S)))
    tiles = ((N + 127) // 128) * ((N + 127) // 128 + 1) // 2
    flop = 3.0 * tiles * 128 * 128 * D            # a subtraction and a fused multiply-add per pair and dimension
    for nk, name in ((8, "pair_all_k_s"), (1, "pair_one_k_s")):
        t = event_time(lambda: pair(nk), args.reps)
        out[name] = t
        out[name.replace("_s", "_fp64_share_of_vector_peak")] = flop / t / FP64_VECTOR_PEAK
    out["pair_fp64_flop"] = flop
    out["pair_algorithmic_bytes"] = N * D * 8 + len(ks) * N * 4
    out["pair_panel_bytes_requested"] = tiles * 2 * 128 * D * 8          # what the tiles load (served by L2 / HBM: not measured)
    out["pair_partial_bytes_written"] = tiles * int((ks.astype(np.int64) ** 2).sum()) * 8
    d_l.free()
    out["sweep_device_s"] = median_time(lambda: audioSegmentation.diarize_clusters_device(d_m, D, N, 0, random_state=3)[1].free(),
                                        max(1, args.reps // 4))
    det, d_z = audioSegmentation.diarize_clusters_device(d_m, D, N, 0, random_state=3)
    d_z.free()
    out["sweep_n_iter"] = {int(k): det["n_iter"][k] for k in det["ks"]}
    d_m.free()
    try:
        out["diarize_features_host_s"] = median_time(lambda: audioSegmentation.diarize_features(M, 0, random_state=3),
                                                     max(1, args.reps // 4))
    except (ValueError, IndexError) as exc:          # a degenerate HMM of the k = 9 labels, as in the reference
        out["diarize_features_host_s"] = "failed: %s" % exc
    out["diarize_features_k6_host_s"] = median_time(lambda: audioSegmentation.diarize_features(M, 6, random_state=3),
                                                    max(1, args.reps // 4))
    # reference-side step 6 on one core: the cdist blocks of one k (N^2 D work: scale by (36 000 / n)^2 for the hour)
    n = args.diar_reference_windows
    Zs, ls = M[:, :n].T.copy(), path[:n] % 4
    t0 = time.perf_counter()
    for c in range(4):
        for c2 in range(4):
            if c != c2:
                np.mean(distance.cdist(Zs[ls == c], Zs[ls == c2]))
    out["reference_cdist_one_k_s"] = time.perf_counter() - t0
    out["reference_cdist_windows"] = n
    # one hour of audio, host to host, seeded SVMs of the shipped shapes
    models = []
    for n_support, seed in ((svc_libsvm.SPEAKER_10_N_SUPPORT, 3), ([120, 120], 4)):
        m = svc_libsvm.synthetic_model(n_support, 136, seed)
        clf = audioTrainTest.SvcArrays(m["support_vectors"], m["n_support"], m["dual_coef"], -m["rho"], m["prob_a"], m["prob_b"],
                                       m["gamma"], "rbf", np.arange(len(m["n_support"]), dtype=np.float64))
        models.append((clf, np.zeros(136), np.ones(136), ["c%d" % i for i in range(len(m["n_support"]))], 1.0, 0.1, 0.05, 0.05,
                       False))
    clip = one_hour_clip()
    for n_speakers in (0, 4):
        key = "one_hour_signal_s_n_speakers_%d" % n_speakers
        try:
            out[key] = median_time(lambda: audioSegmentation.speaker_diarization_signal(clip, 16000, n_speakers, models=models,
                                                                                        random_state=3), 1)
        except (ValueError, IndexError) as exc:
            out[key] = "failed: %s" % exc
    return out


def train(args):
    """evaluate_classifier("knn") at 5 000 x 136, 8 classes, k = 1 .. 15, n_exp = -1 (11 experiments: 88 splits), 90 % training:
    (a) paa_knn_splits_f64 alone on the 88 jobs (one upload of X, one launch); (b) the same jobs as a loop of paa_knn_create +
    paa_knn_predict_f64 + paa_knn_destroy over host-standardised training rows (what the library could do before); (c)
    evaluate_classifier host to host; and one scikit-learn type with the share of its fits.  Wall time around the synchronous
    calls (copies included), the events of paa_timer_* beside it; medians of --train-reps warm calls."""
    import contextlib
    import ctypes as C
    import io
    import train_ref
    from sklearn.preprocessing import StandardScaler
    from pyaudioanalysis_amd import _ffi, audioTrainTest
    _ffi.init(0)
    lib = _ffi.lib()
    feats = train_ref.bench_features()
    names = ["c%d" % c for c in range(len(feats))]
    X, y = train_ref.features_to_matrix(feats)
    X = np.ascontiguousarray(X)
    n_samples, n_dims = X.shape
    params = np.array(train_ref.KNN_PARAMS)
    n_exp = int(50000 / n_samples) + 1
    np.random.seed(7)
    jobs = []
    for k in params:
        for _ in range(n_exp):
            tr, te = audioTrainTest._draw_split(n_samples, 0.9)
            sc = StandardScaler().fit(X[tr])
            jobs.append((tr, te, sc.mean_, sc.scale_, int(k)))
    qpb, tile, step, instances = audioTrainTest.knn_split_geometry()
    out = {"what": "evaluate_classifier('knn'): the split sweep (scripts/bench_classify.py --train)", "samples": n_samples, "dims": n_dims,
           "classes": len(feats), "params": params.tolist(), "n_exp": n_exp, "jobs": len(jobs), "train_percentage": 0.9,
           "queries": int(sum(len(j[1]) for j in jobs)), "train_rows_per_job": int(len(jobs[0][0])),
           "k_instance": int(min(K for K in instances if K >= params.max())),
           "grid_workgroups": int(sum((len(j[1]) + qpb - 1) // qpb for j in jobs)), "threads_per_workgroup": 128,
           "library": os.environ.get("PAA_HIP_LIBRARY", "default"), "reps": args.train_reps}
    out["fp64_flop"] = 3.0 * sum(len(j[0]) * len(j[1]) for j in jobs) * n_dims
    out["bytes_uploaded_sweep"] = int(X.nbytes + 4 * sum(len(j[0]) + len(j[1]) for j in jobs) + 16 * n_dims * len(jobs))
    out["bytes_uploaded_loop"] = int(sum(8 * n_dims * (len(j[0]) + len(j[1])) + 4 * len(j[0]) for j in jobs))

    def both(fn):
        return {"wall_s": median_time(fn, args.train_reps), "events_s": event_time(fn, args.train_reps)}

    # (a) the new entry alone
    res = audioTrainTest.knn_split_predict(X, y, jobs)
    out["a_split_sweep"] = both(lambda: audioTrainTest.knn_split_predict(X, y, jobs))
    out["a_split_sweep"]["note"] = "knn_split_predict: the index lists are concatenated on the host inside the timed call"

    # (b) the loop the library could run before: one uploaded model per split
    lab32 = y.astype(np.int32)
    models = [(np.ascontiguousarray((X[tr] - mean) / scale), np.ascontiguousarray(lab32[tr]), np.ascontiguousarray(X[te].T), mean, scale, k,
               int(np.unique(y[tr]).shape[0])) for tr, te, mean, scale, k in jobs]
    loop_labels = []

    def loop():
        loop_labels.clear()
        for T, lab, Q, mean, scale, k, n_classes in models:
            h = C.c_void_p()
            _ffi.check(lib.paa_knn_create(_ffi.as_f64p(T), lab.ctypes.data_as(_ffi.c_i32p), T.shape[0], n_dims, n_classes, k, C.byref(h)))
            idx = np.empty(Q.shape[1], dtype=np.int32)
            P = np.empty((Q.shape[1], n_classes))
            _ffi.check(lib.paa_knn_predict_f64(h, _ffi.as_f64p(Q), n_dims, Q.shape[1], Q.shape[1], _ffi.as_f64p(mean), _ffi.as_f64p(scale),
                                               idx.ctypes.data_as(_ffi.c_i32p), _ffi.as_f64p(P), None))
            _ffi.check(lib.paa_knn_destroy(h))
            loop_labels.append(idx)
    out["b_model_loop"] = both(loop)
    out["same_labels"] = bool(np.array_equal(np.concatenate(loop_labels), res.label))
    out["loop_over_sweep"] = out["b_model_loop"]["wall_s"] / out["a_split_sweep"]["wall_s"]

    # (c) evaluate_classifier host to host
    def evaluate(kind, p, n):
        np.random.seed(7)
        with contextlib.redirect_stdout(io.StringIO()):
            return audioTrainTest.evaluate_classifier(feats, names, kind, p, 1, None, n_exp=n, train_percentage=0.9)
    out["c_evaluate_classifier_knn"] = {"wall_s": median_time(lambda: evaluate("knn", params, -1), args.train_reps), "best": int(evaluate("knn", params, -1))}

    # one scikit-learn type: where its time goes
    fit_s = [0.0]
    real = audioTrainTest._train_classifier

    def timed_fit(*a):
        t0 = time.perf_counter()
        m = real(*a)
        fit_s[0] += time.perf_counter() - t0
        return m
    audioTrainTest._train_classifier = timed_fit
    try:
        evaluate("randomforest", np.array([25, 100]), 2)
        fit_s[0] = 0.0
        t0 = time.perf_counter()
        evaluate("randomforest", np.array([25, 100]), 2)
        total = time.perf_counter() - t0
    finally:
        audioTrainTest._train_classifier = real
    out["randomforest_25_100_n_exp_2"] = {"wall_s": total, "fits_s": fit_s[0], "fits_share": fit_s[0] / total}
    return out


def reference_loop(args):
    import pickle
    import warnings
    warnings.simplefilter("ignore")
    out = {"reference_sklearn_windows_per_s": {}}
    rng = np.random.default_rng(1)
    for model in MODELS:
        with open(os.path.join(args.reference_loop, model), "rb") as f:
            clf = pickle.load(f)
        X = rng.standard_normal((args.loop_windows, clf.support_vectors_.shape[1]))

        def loop():          # audioSegmentation.py:583-594 -> audioTrainTest.classifier_wrapper (:84-93)
            for v in X:
                clf.predict(v.reshape(1, -1))[0]
                clf.predict_proba(v.reshape(1, -1))[0]
        t = median_time(loop, 3)
        out["reference_sklearn_windows_per_s"][model] = args.loop_windows / t
    out["reference_knn_windows_per_s"] = {}
    from scipy.spatial import distance
    for model in KNN_SHAPES:
        with open(os.path.join(args.reference_loop, model), "rb") as f:
            features, labels = np.array(pickle.load(f)), np.array(pickle.load(f))
            for _ in range(3):          # mean, std, class names
                pickle.load(f)
            k = pickle.load(f)
        n_classes = np.unique(labels).shape[0]
        X = rng.standard_normal((args.loop_windows, features.shape[1]))

        def loop():          # audioSegmentation.py:583-594 -> Knn.classify (audioTrainTest.py:39-49): cdist, argsort, votes
            for v in X:
                order = np.argsort(distance.cdist(features, v.reshape(1, -1), "euclidean").T)
                P = np.array([np.count_nonzero(labels[order[0][:k]] == c) / float(k) for c in range(n_classes)])
                np.argmax(P)
        t = median_time(loop, 3)
        out["reference_knn_windows_per_s"][model] = args.loop_windows / t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--reference-loop", default=None)
    ap.add_argument("--loop-windows", type=int, default=200)
    ap.add_argument("--forest", action="store_true", help="the tree-ensemble shapes only")
    ap.add_argument("--hmm", action="store_true", help="the HMM segmenter only")
    ap.add_argument("--diar", action="store_true", help="speaker diarization only")
    ap.add_argument("--train", action="store_true", help="evaluate_classifier('knn'): the split sweep in one launch")
    ap.add_argument("--train-reps", type=int, default=10)
    ap.add_argument("--diar-windows", type=int, default=36000)
    ap.add_argument("--diar-reference-windows", type=int, default=6000)
    args = ap.parse_args()
    print(json.dumps(reference_loop(args) if args.reference_loop else forest(args) if args.forest else
                     hmm(args) if args.hmm else diar(args) if args.diar else train(args) if args.train else gpu(args)))


if __name__ == "__main__":
    main()
