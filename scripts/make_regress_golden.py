#!/usr/bin/env python3
"""Write tests/golden/svr_*.npz and regforest_*.npz: the regression goldens of the GPU SVR bank (kernels_svr.hpp) and of the
regressor kind of the tree-ensemble kernels (kernels_forest.hpp).

Runs the UNMODIFIED reference (through oracle/load_reference.py, read-only) and the installed scikit-learn on the host.
Every file has a `kind` ("svr" or "regforest"), `sklearn_version`, arrays only (no pickles, no object arrays):

  svr_emotion_files / svr_linear_files / regforest_emotion_files
      the reference's feature_extraction_train_regression on data/speechEmotion (47 clips; arousal and valence) with
      "svm_rbf" / "svm" / "randomforest" under a fixed np.random.seed, models written to a temporary directory; per task
      <t> the model's arrays (SVR: <t>_sv, _coef, _intercept, _gamma, _kernel; forest: <t>_node_offsets ... _value) and
      its MEANS contents (<t>_mean, <t>_std; mt_win, mid_step, st_win, st_step, compute_beat); the int16 signals of four
      clips concatenated (signals, lengths, fs) and the reference's file_regression on each: ref_<t> [n_clips]; the clips'
      long-term vectors (vectors [n_dims][n_clips]) and scikit-learn's predict on them (sk_<t>);
  svr_synth
      seeded scikit-learn SVR fits, rbf and linear, C in {0.001, 1, 10}, one fit whose epsilon leaves no support vector; a
      query matrix X [n_vec][n_dims] and predict of each fit (m<i>_*);
  svr_evaluate
      the reference's evaluate_regression under a fixed seed, n_exp = 5, two parameter values, for "svm" and
      "randomforest": inputs, the returned triple and the printed table.

    python scripts/make_regress_golden.py            # needs the reference tree and scikit-learn
"""
import contextlib
import io
import os
import sys
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import load_reference  # noqa: E402
import svr_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TMP = tempfile.mkdtemp(prefix="regress_golden_")
CLIPS = ("00.wav", "13.wav", "27.wav", "46.wav")
WINDOWS = (1.0, 1.0, 0.05, 0.05)
MAX_BYTES = 997790            # the largest golden in the tree before these


def data(name):
    return os.path.join(load_reference.REFERENCE_ROOT, "pyAudioAnalysis", "data", name)


def reference():
    load_reference.load_segmentation()
    import sklearn
    from pyAudioAnalysis import MidTermFeatures, audioBasicIO, audioTrainTest
    return MidTermFeatures, audioBasicIO, audioTrainTest, sklearn.__version__


def save(name, d):
    path = os.path.join(OUT, "%s.npz" % name)
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    print("%s: %d bytes" % (name, size))
    assert size <= MAX_BYTES, (name, size)


def model_fields(prefix, model_type, model):
    if model_type == "randomforest":
        return {"%s_%s" % (prefix, k): v for k, v in svr_ref.tree_arrays(model).items()}
    sv, coef, intercept, gamma, kernel = svr_ref.svr_arrays(model)
    return {prefix + "_sv": sv, prefix + "_coef": coef, prefix + "_intercept": np.float64(intercept),
            prefix + "_gamma": np.float64(gamma), prefix + "_kernel": np.str_(kernel)}


def emotion_case(name, kind, model_type, seed):
    mtf, io_, at, version = reference()
    model_name = os.path.join(TMP, name)
    np.random.seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        at.feature_extraction_train_regression(data("speechEmotion"), *WINDOWS, model_type, model_name, False)
    d = {"kind": np.str_(kind), "model_type": np.str_(model_type), "sklearn_version": np.str_(version), "seed": np.int64(seed)}
    sigs, vecs = [], []
    results = {}
    for clip in CLIPS:
        with contextlib.redirect_stdout(io.StringIO()):
            R, names = at.file_regression(data(os.path.join("speechEmotion", clip)), model_name, model_type)
        for r, t in zip(R, names):
            results.setdefault(t, []).append(r)
        fs, sig = io_.read_audio_file(data(os.path.join("speechEmotion", clip)))
        sig = io_.stereo_to_mono(sig)
        assert sig.dtype == np.int16
        sigs.append(sig)
        mt, _, _ = mtf.mid_feature_extraction(sig, fs, WINDOWS[0] * fs, WINDOWS[1] * fs, round(fs * WINDOWS[2]), round(fs * WINDOWS[3]))
        vecs.append(mt.mean(axis=1))
    tasks = sorted(results)
    d.update({"tasks": np.array(tasks, dtype=np.str_), "signals": np.concatenate(sigs),
              "lengths": np.array([len(s) for s in sigs], dtype=np.int64), "fs": np.float64(fs),
              "vectors": np.stack(vecs, axis=1)})
    for t in tasks:
        model, mean, std, mt_win, mid_step, st_win, st_step, beat = at.load_model(model_name + "_" + t, True)
        d.update(model_fields(t, model_type, model))
        d.update({t + "_mean": mean, t + "_std": std, "mt_win": np.float64(mt_win), "mid_step": np.float64(mid_step),
                  "st_win": np.float64(st_win), "st_step": np.float64(st_step), "compute_beat": np.bool_(beat),
                  "ref_" + t: np.array(results[t], dtype=np.float64),
                  "sk_" + t: model.predict((d["vectors"].T - mean) / std)})
    save(name, d)


def synth_case():
    import sklearn
    from sklearn.svm import SVR
    rng = np.random.default_rng(31)
    n_dims = 23
    Xtr = rng.standard_normal((120, n_dims))
    y = Xtr[:, :5] @ rng.standard_normal(5) + 0.3 * np.sin(Xtr[:, 5]) + 0.1 * rng.standard_normal(120)
    X = rng.standard_normal((77, n_dims))
    d = {"kind": np.str_("svr"), "case": np.str_("synth"), "sklearn_version": np.str_(sklearn.__version__), "X": X}
    fits = [(k, c, 0.1) for k in ("rbf", "linear") for c in (0.001, 1.0, 10.0)] + [("rbf", 1.0, 1e3)]
    for i, (kernel, c, eps) in enumerate(fits):
        model = SVR(kernel=kernel, C=c, epsilon=eps).fit(Xtr, y)
        d.update(model_fields("m%d" % i, "svm", model))
        d["m%d_predict" % i] = model.predict(X)
        print("synth", kernel, c, eps, "support vectors", model.support_vectors_.shape[0])
    assert d["m6_sv"].shape[0] == 0
    d["n_models"] = np.int64(len(fits))
    save("svr_synth", d)


def evaluate_case():
    _, _, at, version = reference()
    rng = np.random.default_rng(32)
    features = rng.standard_normal((40, 12)) * rng.uniform(0.5, 3.0, 12) + rng.standard_normal(12)
    labels = features[:, :4] @ rng.standard_normal(4) + 0.2 * rng.standard_normal(40)
    d = {"kind": np.str_("svr"), "case": np.str_("evaluate"), "sklearn_version": np.str_(version), "features": features,
         "labels": labels, "n_exp": np.int64(5), "seed": np.int64(77)}
    for method, params in (("svm", np.array([0.1, 1.0])), ("randomforest", np.array([5, 10]))):
        np.random.seed(77)
        with contextlib.redirect_stdout(io.StringIO()) as printed:
            best, err, base = at.evaluate_regression(features, labels, 5, method, params)
        d.update({method + "_params": params, method + "_result": np.array([best, err, base], dtype=np.float64),
                  method + "_printed": np.str_(printed.getvalue())})
    save("svr_evaluate", d)


def main():
    warnings.simplefilter("ignore")
    synth_case()
    evaluate_case()
    emotion_case("svr_emotion_files", "svr", "svm_rbf", 11)
    emotion_case("svr_linear_files", "svr", "svm", 12)
    emotion_case("regforest_emotion_files", "regforest", "randomforest", 13)


if __name__ == "__main__":
    main()
