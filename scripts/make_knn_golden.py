#!/usr/bin/env python3
"""Write tests/golden/knn_*.npz: the classification goldens of the GPU kNN kernel (kernels_knn.hpp).

Runs the UNMODIFIED reference (through oracle/load_reference.py, read-only) on the host.  Every file has kind = "knn", no
object arrays (class names are a fixed-width unicode array) and holds one model in load_model_knn's terms (features,
labels, neighbors, mean, std, class names, windows and steps, compute_beat) and a feature matrix `mid` [n_dims][n_vec]
(raw, standardised with mean / std by the consumer) with the reference's Knn.classify answers on it (ref_labels, ref_P),
a flag per vector whose vote set the reference's unstable argsort leaves undefined (ref_ambiguous, from the reference's
own cdist distances: tests/knn_ref.ambiguous) and the answers under the documented (squared distance, index) order
(want_labels, want_P, want_nb: tests/knn_ref.py).  Cases:

  segment  knn_sm_speech_music, knn_malefemale_diarization: a seeded subset of a shipped model's rows (its own labels, k,
           mean and std; the full models are too large for a golden file) written in load_model_knn's format; the
           reference's mid_term_file_classification on the signal; `mid` is the signal's mid-term matrix at a 0.1 s step
  matrix   knn_sm_dense_diarization: the knn_sm subset on 30 s of diarizationExample.wav at a 0.1 s step
  file     knn_genre6_files: the real knn_musical_genre_6 (138 dims, beat); the reference's file_classification on cuts of
           doremi.wav and count.wav; `mid` holds their long-term vectors
  ties     knn_ties, knn_ties_short: small integer-valued models with exact distances -- duplicated rows with different
           labels, exact ties at the k boundary, a label outside 0..n_classes-1, a class no query gets, n_train < k

    python scripts/make_knn_golden.py            # needs the reference tree
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
import knn_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TMP = "/tmp"
SUBSET_ROWS = 450


def data(name):
    return os.path.join(load_reference.REFERENCE_ROOT, "pyAudioAnalysis", "data", name)


def model_path(name):
    return data(os.path.join("models", name))


def reference():
    seg = load_reference.load_segmentation()
    from pyAudioAnalysis import MidTermFeatures, audioBasicIO, audioTrainTest
    return seg, MidTermFeatures, audioBasicIO, audioTrainTest


def write_knn_model(path, features, labels, mean, std, classes, k, mt_win, mid_step, st_win, st_step, compute_beat):
    """A model file in load_model_knn's format (eleven pickles in its order)."""
    with open(path, "wb") as f:
        for obj in (features, labels, mean, std, classes, k, mt_win, mid_step, st_win, st_step, compute_beat):
            pickle.dump(obj, f, protocol=pickle.HIGHEST_PROTOCOL)


def subset_model(name, seed):
    """A seeded subset of a shipped model's rows in load_model_knn's format; returns (path, the loaded tuple)."""
    _, _, _, at = reference()
    clf, mean, std, classes, mt_win, mid_step, st_win, st_step, beat = at.load_model_knn(model_path(name))
    rng = np.random.default_rng(seed)
    keep = np.sort(rng.choice(clf.features.shape[0], SUBSET_ROWS, replace=False))
    path = os.path.join(TMP, "knn_golden_%s_subset" % name)
    write_knn_model(path, clf.features[keep], clf.labels[keep], mean, std, classes, clf.neighbors, mt_win, mid_step, st_win,
                    st_step, beat)
    return path, at.load_model_knn(path)


def model_fields(loaded, name):
    clf, mean, std, classes, mt_win, mid_step, st_win, st_step, beat = loaded
    return {"kind": np.str_("knn"), "model": np.str_(name), "features": np.asarray(clf.features, dtype=np.float64),
            "labels": np.asarray(clf.labels, dtype=np.float64), "neighbors": np.int64(clf.neighbors),
            "mean": np.asarray(mean, dtype=np.float64), "std": np.asarray(std, dtype=np.float64),
            "class_names": np.array(classes, dtype=np.str_), "mt_win": np.float64(mt_win), "mid_step": np.float64(mid_step),
            "st_win": np.float64(st_win), "st_step": np.float64(st_step), "compute_beat": np.bool_(beat)}


def matrix_fields(clf, mid, mean, std):
    """The reference's Knn.classify on every column of mid, its ambiguity flags, and the restatement's answers."""
    from scipy.spatial import distance
    X = ((mid.T - mean) / std)
    ref_labels, ref_P, amb = [], [], []
    for x in X:
        c, p = clf.classify(x)
        ref_labels.append(c)
        ref_P.append(p)
        amb.append(knn_ref.ambiguous(distance.cdist(clf.features, x.reshape(1, -1), "euclidean")[:, 0], clf.labels,
                                     clf.neighbors))
    want_labels, want_P, want_nb = knn_ref.classify(clf.features, clf.labels, clf.neighbors, X)
    return {"mid": np.ascontiguousarray(mid, dtype=np.float64), "ref_labels": np.array(ref_labels, dtype=np.int64),
            "ref_P": np.array(ref_P, dtype=np.float64), "ref_ambiguous": np.array(amb, dtype=bool),
            "want_labels": want_labels, "want_P": want_P, "want_nb": want_nb}


def mid_matrix(sig, fs, mt_win, step, st_win, st_step):
    _, mtf, _, _ = reference()
    mt, _, _ = mtf.mid_feature_extraction(sig, fs, mt_win * fs, step * fs, round(fs * st_win), round(fs * st_step))
    return mt


def save(name, d):
    path = os.path.join(OUT, "%s.npz" % name)
    np.savez_compressed(path, **d)
    print("%s: %d vectors, %d ambiguous, %d bytes" % (name, d["mid"].shape[1], int(d["ref_ambiguous"].sum()),
                                                       os.path.getsize(path)))


def segment_case(name, wav, model, seed, gt=None, seconds=None):
    ref_seg, _, io_, _ = reference()
    path_model, loaded = subset_model(model, seed)
    clf, mean, std, class_names, mt_win, mid_step, st_win, st_step, _ = loaded
    fs, sig = io_.read_audio_file(data(wav))
    sig = io_.stereo_to_mono(sig)
    path = data(wav)
    if seconds is not None:                      # a cut of the file, written where the reference can read it
        import scipy.io.wavfile as wavfile
        sig = sig[:int(seconds * fs)]
        path = os.path.join(TMP, "knn_golden_%s.wav" % name)
        wavfile.write(path, fs, sig)
    with contextlib.redirect_stdout(io.StringIO()) as printed:
        labels, cn, acc, cm = ref_seg.mid_term_file_classification(path, path_model, "knn", False, data(gt) if gt else "")
    d = model_fields(loaded, model)
    d.update({"case": np.str_("segment"), "signal": sig, "fs": np.float64(fs),
              "seg_labels": np.asarray(labels, dtype=np.int64), "ref_accuracy": np.float64(acc), "ref_cm": np.asarray(cm),
              "ref_printed": np.str_(printed.getvalue())})
    if gt:
        s, e, lab = ref_seg.read_segmentation_gt(data(gt))
        _, names_gt = ref_seg.segments_to_labels(s, e, lab, mid_step)
        d["gt_segments"] = np.array([[a, b] for a, b in zip(s, e)])
        d["gt_labels"] = np.array(lab, dtype=np.str_)
        d["ref_class_names_gt"] = np.array(names_gt, dtype=np.str_)      # the row / column order of ref_cm (a set's order)
    d.update(matrix_fields(clf, mid_matrix(sig, fs, mt_win, 0.1, st_win, st_step), mean, std))
    save("knn_" + name, d)


def dense_case(name, wav, model, seed, seconds):
    _, _, io_, _ = reference()
    _, loaded = subset_model(model, seed)
    clf, mean, std, _, mt_win, _, st_win, st_step, _ = loaded
    fs, sig = io_.read_audio_file(data(wav))
    sig = io_.stereo_to_mono(sig)[:int(seconds * fs)]
    d = model_fields(loaded, model)
    d["case"] = np.str_("matrix")
    d.update(matrix_fields(clf, mid_matrix(sig, fs, mt_win, 0.1, st_win, st_step), mean, std))
    save("knn_" + name, d)


def file_case(name, cuts, model):
    _, mtf, io_, at = reference()
    import scipy.io.wavfile as wavfile
    loaded = at.load_model_knn(model_path(model))
    clf, mean, std, class_names, mt_win, mid_step, st_win, st_step, beat = loaded
    sigs, ids, probs, vecs = [], [], [], []
    for wav, seconds in cuts:
        fs, sig = io_.read_audio_file(data(wav))
        sig = io_.stereo_to_mono(sig)[:int(seconds * fs)]
        path = os.path.join(TMP, "knn_golden_%s_%s" % (name, wav))
        wavfile.write(path, fs, sig)
        cid, p, classes = at.file_classification(path, model_path(model), "knn")
        sigs.append(sig)
        ids.append(cid)
        probs.append(p)
        # the long-term vector file_classification classifies (reference :1077-1090)
        mw = min(mt_win, sig.shape[0] / float(fs))
        mt, s, _ = mtf.mid_feature_extraction(sig, fs, mw * fs, mid_step * fs, round(fs * st_win), round(fs * st_step))
        v = mt.mean(axis=1)
        if beat:
            b, bc = mtf.beat_extraction(s, st_step)
            v = np.append(np.append(v, b), bc)
        vecs.append(v)
    d = model_fields(loaded, model)
    d.update({"case": np.str_("file"), "signals": np.concatenate(sigs), "lengths": np.array([len(s) for s in sigs]),
              "fs": np.float64(fs), "ref_ids": np.array(ids, dtype=np.int64), "ref_proba": np.array(probs)})
    d.update(matrix_fields(clf, np.stack(vecs, axis=1), mean, std))
    assert np.array_equal(d["ref_labels"], d["ref_ids"]) and np.array_equal(d["ref_P"], d["ref_proba"])
    save("knn_" + name, d)


def ties_case(name, features, labels, k, queries, classes):
    _, _, _, at = reference()
    n_dims = features.shape[1]
    clf = at.Knn(np.asarray(features, dtype=np.float64), np.asarray(labels, dtype=np.float64), k)
    loaded = (clf, np.zeros(n_dims), np.ones(n_dims), classes, 1.0, 1.0, 0.05, 0.05, False)
    d = model_fields(loaded, name)
    d["case"] = np.str_("ties")
    d.update(matrix_fields(clf, np.asarray(queries, dtype=np.float64).T, np.zeros(n_dims), np.ones(n_dims)))
    save("knn_" + name, d)


def main():
    warnings.simplefilter("ignore")
    segment_case("sm_speech_music", "speech_music_sample.wav", "knn_sm", 1)
    segment_case("malefemale_diarization", "diarizationExample.wav", "knn_speaker_male_female", 2,
                 gt="diarizationExample.segments", seconds=8)
    dense_case("sm_dense_diarization", "diarizationExample.wav", "knn_sm", 1, 30)
    file_case("genre6_files", [("doremi.wav", 3.5), ("count.wav", 3.0)], "knn_musical_genre_6")
    rng = np.random.default_rng(31)
    # 14 integer rows in 3 dims: rows 0 / 1 and 6 / 7 are duplicates with different labels, label 5 is outside
    # 0..n_classes-1 (n_classes = 4 distinct labels: 0, 1, 2, 5), class 3 does not exist, so no query gets it
    feats = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 2, 0], [2, 2, 0], [-1, -1, 0],
                      [3, 0, 1], [0, -2, 2], [1, 1, 1], [-2, 0, -1], [0, 3, -1], [1, -1, -1]], dtype=np.float64)
    labels = np.array([0, 1, 0, 1, 2, 1, 2, 5, 0, 2, 1, 0, 5, 2], dtype=np.float64)
    queries = np.concatenate([rng.integers(-3, 4, (300, 3)), feats, np.zeros((1, 3))]).astype(np.float64)
    ties_case("ties", feats, labels, 4, queries, ["a", "b", "c", "d"])
    # fewer rows than neighbours: P is still divided by k
    short = np.array([[0, 0], [1, 1], [4, 0]], dtype=np.float64)
    ties_case("ties_short", short, np.array([0, 1, 1], dtype=np.float64), 5,
              rng.integers(-2, 5, (40, 2)).astype(np.float64), ["a", "b"])


if __name__ == "__main__":
    main()
