#!/usr/bin/env python3
"""Write tests/golden/lda_*.npz: the goldens of the LDA branch of GPU speaker diarization (kernels_lda.hpp).

The input X (n windows x D) of the real-audio cases comes from the UNMODIFIED reference (through oracle/load_reference.py,
read-only): its short-term features, the step-1 mid-term statistics, the predict_proba of the two shipped speaker SVMs + 1e-4
and StandardScaler, as speaker_diarization assembles them for lda_dim > 0.  The expected outputs are scikit-learn's:
LinearDiscriminantAnalysis(n_components).fit (xbar_, scalings_, transform), then KMeans(n_clusters=k, init=centres, n_init=1),
the reference's silhouette and scipy.signal.medfilt.  An SVD leaves the sign of every column open; the golden fixes it --
largest-magnitude entry of every scalings_ column positive -- BEFORE the later stages run, as the package does.  The NumPy
restatement tests/lda_ref.py must agree with scikit-learn (1e-9), and the margins of every decision are stored with the
results; a seed is skipped when a k-means or silhouette decision of its run is closer to a tie than the floor.
Of the Gram matrix every 7th row is stored (the tests restate the whole of it from X with tests/lda_ref.py).
kind = "lda", no object arrays, no pickle, every file under 700 KB.  Cases:

  lda_example     the first 24 s of diarizationExample.wav, mid_window 1.0, short_window 0.2 (25-window classes, a short last one), lda_dim 12
  lda_example2    the first 24 s of diarizationExample2.wav, the same settings
  lda_synth       planted speakers, unequal runs, one run of a single window, one constant dimension, lda_dim 6

    python scripts/make_lda_golden.py            # needs the reference tree and scikit-learn
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import load_reference  # noqa: E402
import diar_ref  # noqa: E402
import lda_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
DIST_FLOOR = 1e-6
RANK_FLOOR = 10.0
KS = list(range(2, 10))
CLS_KS = (4, 9)
TIGHT = 1e-9


def data(name):
    return os.path.join(load_reference.REFERENCE_ROOT, "pyAudioAnalysis", "data", name)


def reference_matrix(wav, seconds, mid_window, short_window):
    """(X [T][148], labels [T]) as speaker_diarization builds them for lda_dim > 0."""
    from pyAudioAnalysis import audioTrainTest as at
    from pyAudioAnalysis import MidTermFeatures as mtf
    from pyAudioAnalysis import audioBasicIO as io
    from sklearn.preprocessing import StandardScaler
    fs, x = io.read_audio_file(data(wav))
    x = io.stereo_to_mono(x)[:int(seconds * fs)]
    models = [at.load_model(data(os.path.join("models", n))) for n in ("svm_rbf_speaker_10", "svm_rbf_speaker_male_female")]
    _, st, _ = mtf.mid_feature_extraction(x, fs, mid_window * fs, 0.1 * fs, round(fs * 0.05), round(fs * 0.05))
    ratio = int(round(mid_window / short_window))
    T = st.shape[1]
    stats = np.vstack([np.stack([st[:, t:t + ratio].mean(axis=1) for t in range(T)], axis=1),
                       np.stack([st[:, t:t + ratio].std(axis=1) for t in range(T)], axis=1)])
    blocks = [stats]
    for clf, mean, std, names, _, _, _, _, _ in models:
        P = np.empty((len(names), T))
        for i in range(T):
            P[:, i] = at.classifier_wrapper(clf, "svm_rbf", (stats[:, i] - mean) / std)[1] + 1e-4
        blocks.append(P)
    X = StandardScaler().fit_transform(np.vstack(blocks).T)
    return np.ascontiguousarray(X), lda_ref.window_labels(T, short_window)


def close(x, ref):
    return np.max(np.abs(np.asarray(x) - np.asarray(ref))) <= TIGHT * max(np.max(np.abs(ref)), 1.0)


def sk_silhouette(Y, cls, k):
    from scipy.spatial import distance
    a, b = np.zeros(k), np.zeros(k)
    for c in range(k):
        share = np.nonzero(cls == c)[0].shape[0] / float(len(cls))
        if share < 0.020:
            continue
        mine = Y[cls == c, :]
        a[c] = np.mean(distance.pdist(mine.T)) * share
        cand = []
        for c2 in range(k):
            if c2 != c:
                share2 = np.nonzero(cls == c2)[0].shape[0] / float(len(cls))
                cand.append(np.mean(distance.cdist(mine, Y[cls == c2, :])) * (share + share2) / 2.0)
        b[c] = min(cand)
    sil = np.array([(b[c] - a[c]) / (max(b[c], a[c]) + 1e-5) for c in range(k)])
    return a, b, sil


def run_k(Y, k, seed):
    from sklearn.cluster import KMeans, kmeans_plusplus
    init, _ = kmeans_plusplus(Y, k, random_state=seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = KMeans(n_clusters=k, init=init, n_init=1).fit(Y)
    r = diar_ref.kmeans(Y, k, init)
    if r["margin"] < DIST_FLOOR or not np.array_equal(r["labels"], km.labels_) or r["n_iter"] != km.n_iter_:
        return None
    if not close(r["centers"], km.cluster_centers_) or not close(r["inertia"], km.inertia_):
        return None
    a, b, sil = sk_silhouette(Y, km.labels_, k)
    s = diar_ref.silhouette(Y, r["labels"], k)
    if s["b_margin"] < DIST_FLOOR or not (close(s["a"], a) and close(s["b"], b) and close(s["sil"], sil)):
        return None
    return {"seed": seed, "init": init, "labels": km.labels_.astype(np.int16), "centers": km.cluster_centers_, "n_iter": km.n_iter_,
            "inertia": km.inertia_, "a": a, "b": b, "sil": sil, "km_margin": r["margin"], "b_margin": s["b_margin"],
            "pair_sums": diar_ref.pair_sums(Y, km.labels_, k)}


def make_case(name, X, labels, dim):
    from scipy.signal import medfilt
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
    clf = LinearDiscriminantAnalysis(n_components=dim).fit(X, labels)
    scal, flips, _ = lda_ref.sign_fix(clf.scalings_[:, :dim])
    Y = np.ascontiguousarray(clf.transform(X) * flips)
    r = lda_ref.fit(X, labels, dim)
    assert close(r["xbar"], clf.xbar_) and close(r["means"], clf.means_) and close(r["scalings"], scal) and close(r["Y"], Y), name
    assert min(r["rank_margin"]) >= RANK_FLOOR and min(r["rank2_margin"]) >= RANK_FLOOR, (name, r["rank_margin"], r["rank2_margin"])
    assert r["s2_gap"] >= DIST_FLOOR and r["sign_margin"] >= DIST_FLOOR, (name, r["s2_gap"], r["sign_margin"])
    g = {"kind": np.array("lda"), "X": X, "labels": labels.astype(np.int32), "dim": np.array(dim), "xbar": clf.xbar_,
         "means": clf.means_, "std": r["std"], "gram_sample": r["gram"][::7], "scalings": scal, "Y": Y, "S": r["S"], "S2": r["S2"],
         "rank": np.array(r["rank"]), "rank2": np.array(r["rank2"]), "rank_margin": np.array(r["rank_margin"]),
         "rank2_margin": np.array(r["rank2_margin"]), "s2_gap": np.array(r["s2_gap"]), "sign_margin": np.array(r["sign_margin"]),
         "ks": np.array(KS), "cls_ks": np.array(CLS_KS)}
    scores = []
    for k in KS:
        for seed in range(200):
            rk = run_k(Y, k, seed)
            if rk is not None:
                break
        else:
            raise SystemExit("%s: no usable seed for k = %d" % (name, k))
        if k in CLS_KS:
            rk["cls"] = medfilt(rk["labels"].astype(np.float64), 5)
        for key, v in rk.items():
            g["k%d_%s" % (k, key)] = np.asarray(v)
        scores.append(np.mean(rk["sil"]))
        print("  %s k=%d seed=%d n_iter=%d margins km %.2e b %.2e" % (name, k, rk["seed"], rk["n_iter"], rk["km_margin"], rk["b_margin"]))
    top = np.sort(scores)[-2:]
    assert top[1] - top[0] >= DIST_FLOOR, (name, "imax", top)
    g["scores"] = np.array(scores)
    g["imax"] = np.array(int(np.argmax(scores)))
    g["imax_margin"] = np.array(top[1] - top[0])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **g)
    size = os.path.getsize(path)
    assert size < 700000, (name, size)
    print("wrote %s: n x D = %s, %d classes, rank %d / %d, margins %s %s, gap %.2e, sign %.2e, %d bytes" % (
        name, X.shape, labels.max() + 1, r["rank"], r["rank2"], r["rank_margin"], r["rank2_margin"], r["s2_gap"], r["sign_margin"], size))


def synthetic(seed=11):
    """Planted speakers in 40 dims, 23 runs of unequal length with one run of a single window, one constant dimension."""
    rng = np.random.default_rng(seed)
    runs = [int(v) for v in rng.integers(8, 60, 22)]
    runs.insert(9, 1)
    X, labels = lda_ref.planted(seed, sum(runs), 40, runs)
    X[:, 17] = 3.25
    return np.ascontiguousarray(X), labels


def main():
    if not load_reference.reference_available():
        raise SystemExit("the reference tree is needed")
    load_reference.load_segmentation()
    os.makedirs(OUT, exist_ok=True)
    X, labels = reference_matrix("diarizationExample.wav", 24, 1.0, 0.2)
    make_case("lda_example", X, labels, 12)
    X, labels = reference_matrix("diarizationExample2.wav", 24, 1.0, 0.2)
    make_case("lda_example2", X, labels, 12)
    X, labels = synthetic()
    make_case("lda_synth", X, labels, 6)


if __name__ == "__main__":
    main()
