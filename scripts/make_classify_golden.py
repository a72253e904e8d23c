#!/usr/bin/env python3
"""Write tests/golden/svc_*.npz: the classification goldens of the GPU SVC (kernels_svc.hpp).

Runs the UNMODIFIED reference (through oracle/load_reference.py, read-only) and the installed scikit-learn on the host:
for each case the input signal (or feature matrix), the model's arrays in libsvm's layout (support vectors, n_support,
_dual_coef_, rho = -_intercept_, probA_ / probB_, gamma, kernel, classes_), the standardised vectors' scikit-learn
predict / predict_proba / decision values, and the reference's mid_term_file_classification / file_classification
outputs.  Every file has kind = "svc" and no object arrays (class names are a fixed-width unicode array).

    python scripts/make_classify_golden.py            # needs the reference tree and scikit-learn
"""
import contextlib
import io
import os
import pickle
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import load_reference  # noqa: E402
import svc_libsvm  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def data(name):
    return os.path.join(load_reference.REFERENCE_ROOT, "pyAudioAnalysis", "data", name)


def model_path(name):
    return data(os.path.join("models", name))


def model_fields(clf, prefix=""):
    m = svc_libsvm.model_arrays(clf)
    return {"sv": m["support_vectors"], "n_support": m["n_support"], "dual_coef": m["dual_coef"], "rho": m["rho"],
            "prob_a": m["prob_a"], "prob_b": m["prob_b"], "gamma": np.float64(m["gamma"]), "kernel": np.str_(m["kernel"]),
            "classes": np.asarray(clf.classes_, dtype=np.float64)}


def sklearn_outputs(clf, X):
    """X: standardised vectors [n_vec][n_dims]."""
    dec = np.stack([svc_libsvm.decision_values(svc_libsvm.model_arrays(clf), X)])[0]
    return {"sk_labels": clf.predict(X).astype(np.float64), "sk_proba": clf.predict_proba(X), "sk_dec": dec}


def segment_case(name, wav, model, gt=None, seconds=None):
    ref_seg = load_reference.load_segmentation()
    from pyAudioAnalysis import MidTermFeatures as mtf, audioBasicIO, audioTrainTest as at
    clf, mean, std, class_names, mt_win, mid_step, st_win, st_step, compute_beat = at.load_model(model_path(model))
    fs, sig = audioBasicIO.read_audio_file(data(wav))
    sig = audioBasicIO.stereo_to_mono(sig)
    path = data(wav)
    if seconds is not None:                      # a cut of the file, written where the reference can read it
        import scipy.io.wavfile as wavfile
        sig = sig[:int(seconds * fs)]
        path = os.path.join("/tmp", "svc_golden_%s.wav" % name)
        wavfile.write(path, fs, sig)
    with contextlib.redirect_stdout(io.StringIO()) as printed:
        labels, cn, acc, cm = ref_seg.mid_term_file_classification(path, model_path(model), "svm_rbf", False,
                                                                   data(gt) if gt else "")
    mt, _, _ = mtf.mid_feature_extraction(sig, fs, mt_win * fs, mid_step * fs, round(fs * st_win), round(fs * st_step))
    X = ((mt.T - mean) / std)
    d = {"kind": np.str_("svc"), "case": np.str_("segment"), "model": np.str_(model), "signal": sig, "fs": np.float64(fs),
         "mean": mean, "std": std, "class_names": np.array(class_names, dtype=np.str_), "mt_win": np.float64(mt_win),
         "mid_step": np.float64(mid_step), "st_win": np.float64(st_win), "st_step": np.float64(st_step), "mid": mt,
         "ref_labels": np.asarray(labels, dtype=np.float64), "ref_accuracy": np.float64(acc), "ref_cm": np.asarray(cm),
         "ref_printed": np.str_(printed.getvalue())}
    if gt:
        s, e, lab = ref_seg.read_segmentation_gt(data(gt))
        _, names_gt = ref_seg.segments_to_labels(s, e, lab, mid_step)
        d["gt_segments"] = np.array([[a, b] for a, b in zip(s, e)])
        d["gt_labels"] = np.array(lab, dtype=np.str_)
        d["ref_class_names_gt"] = np.array(names_gt, dtype=np.str_)      # the row / column order of ref_cm (a set's order)
    d.update(model_fields(clf))
    d.update(sklearn_outputs(clf, X))
    np.savez_compressed(os.path.join(OUT, "svc_%s.npz" % name), **d)
    print(name, "windows", X.shape[0], "classes", len(class_names), "accuracy", acc)


def file_case(name, wavs, model):
    load_reference.load_segmentation()
    from pyAudioAnalysis import MidTermFeatures as mtf, audioBasicIO, audioTrainTest as at
    clf, mean, std, class_names, mt_win, mid_step, st_win, st_step, compute_beat = at.load_model(model_path(model))
    sigs, ids, probs, vecs = [], [], [], []
    for w in wavs:
        cid, p, classes = at.file_classification(data(w), model_path(model), "svm_rbf")
        fs, sig = audioBasicIO.read_audio_file(data(w))
        sigs.append(audioBasicIO.stereo_to_mono(sig))
        ids.append(cid)
        probs.append(p)
    lens = np.array([len(s) for s in sigs], dtype=np.int64)
    d = {"kind": np.str_("svc"), "case": np.str_("file"), "model": np.str_(model), "signals": np.concatenate(sigs),
         "lengths": lens, "fs": np.float64(fs), "mean": mean, "std": std, "class_names": np.array(class_names, dtype=np.str_),
         "mt_win": np.float64(mt_win), "mid_step": np.float64(mid_step), "st_win": np.float64(st_win),
         "st_step": np.float64(st_step), "compute_beat": np.bool_(compute_beat), "ref_ids": np.array(ids, dtype=np.float64),
         "ref_proba": np.array(probs)}
    d.update(model_fields(clf))
    np.savez_compressed(os.path.join(OUT, "svc_%s.npz" % name), **d)
    print(name, "files", len(wavs), ids)


def linear_case():
    from sklearn.svm import SVC
    rng = np.random.default_rng(2024)
    n_dims, k = 136, 3
    centres = rng.standard_normal((k, n_dims))
    y = rng.integers(0, k, 240)
    X = centres[y] * 0.6 + rng.standard_normal((240, n_dims))
    clf = SVC(kernel="linear", probability=True, C=1.0, random_state=0).fit(X, y)
    m = svc_libsvm.model_arrays(clf)
    # test vectors: random ones plus points between the class centres, where the three pairwise votes can form a cycle
    T = rng.standard_normal((600, n_dims)) * 0.8 + (centres[rng.integers(0, k, 600)] * 0.2)
    dec = svc_libsvm.decision_values(m, T)
    votes = np.zeros((T.shape[0], k), dtype=int)
    p = 0
    for i in range(k):
        for j in range(i + 1, k):
            votes[dec[:, p] > 0, i] += 1
            votes[dec[:, p] <= 0, j] += 1
            p += 1
    tie = np.all(votes == 1, axis=1)
    keep = np.concatenate([np.nonzero(tie)[0], np.nonzero(~tie)[0][:200]])
    T = T[keep]
    mean = rng.standard_normal(n_dims) * 0.1
    std = rng.uniform(0.5, 2.0, n_dims)
    mid = (T * std + mean).T                      # feature-major, so that (mid - mean) / std is T (up to rounding)
    X = ((mid.T - mean) / std)
    d = {"kind": np.str_("svc"), "case": np.str_("matrix"), "model": np.str_("linear3"), "mid": mid, "mean": mean, "std": std,
         "class_names": np.array(["a", "b", "c"], dtype=np.str_), "n_tied_votes": np.int64(tie.sum())}
    d.update(model_fields(clf))
    d.update(sklearn_outputs(clf, X))
    np.savez_compressed(os.path.join(OUT, "svc_linear3_ties.npz"), **d)
    print("linear3 vectors", X.shape[0], "tied votes", int(tie.sum()))


def main():
    warnings.simplefilter("ignore")
    segment_case("sm_speech_music", "speech_music_sample.wav", "svm_rbf_sm")
    segment_case("malefemale_diarization", "diarizationExample.wav", "svm_rbf_speaker_male_female",
                 gt="diarizationExample.segments", seconds=8)
    file_case("genre6_files", ["doremi.wav", "count.wav"], "svm_rbf_musical_genre_6")
    # svm_rbf_speaker_10 and svm_rbf_movie8class are not written: their support vectors alone (1.1 MB, 2.5 MB of
    # incompressible float64) exceed what one golden file may hold.  tests/test_svc_cpu.py checks the restatement against
    # scikit-learn on those two models where the reference tree is present, and the GPU tests run seeded models of exactly
    # their shape (svc_libsvm.synthetic_model) against the restatement.
    linear_case()


if __name__ == "__main__":
    main()
