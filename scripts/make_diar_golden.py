#!/usr/bin/env python3
"""Write tests/golden/diar_*.npz: the goldens of GPU speaker diarization (kernels_diar.hpp).

Runs the UNMODIFIED reference (through oracle/load_reference.py, read-only) on the host for the input matrix M (D x N):
mid_feature_extraction and the predict_proba of the two shipped speaker SVMs + 1e-4, exactly as speaker_diarization
assembles it.  The expected output of every later stage comes from the SciPy / scikit-learn calls the reference makes
(StandardScaler, pdist, cdist, KMeans(n_clusters=k, init=centres, n_init=1), medfilt); the HMM step has no live reference
here (hmmlearn is not installed): tests/hmm_ref.py stands in.  The initial centres of every k come from
sklearn.cluster.kmeans_plusplus with a recorded seed.  The margins of every decision (tests/diar_ref.py) are stored with the
results; a seed is skipped when a k-means, silhouette or HMM decision of its run is closer to a tie than the floors below, when
diar_ref and scikit-learn disagree, or when its HMM is degenerate (a cluster with a zero deviation or a state never left).
kind = "diar", no object arrays, no pickle, every file under 1 MB.  Cases:

  diar_example      diarizationExample.wav, mid-term 1.0 / 0.1 s (420 windows); the k = 4 seed is one whose run reaches both
                    purities >= 0.9
  diar_example_2s   the same file at 2.0 / 0.2 s (the settings of speaker_diarization_evaluation)
  diar_example2     diarizationExample2.wav, 1.0 / 0.1 s (223 windows)
  diar_synth        planted clusters, a block of exactly repeated windows, one cluster under the 2 % share
  diar_const        a constant row (clustering stages only: the HMM refuses the zero deviation)

    python scripts/make_diar_golden.py            # needs the reference tree
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
import hmm_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
DIST_FLOOR = 1e-6          # relative gap of the distance-based decisions (steps 4, 5, 6)
HMM_FLOOR = 1e-3           # nats
KS = list(range(2, 10))
TIGHT = 1e-9


def data(name):
    return os.path.join(load_reference.REFERENCE_ROOT, "pyAudioAnalysis", "data", name)


def reference_matrix(ref_seg, wav, mid_window, mid_step):
    """M as speaker_diarization builds it (:828-859) and the ground-truth flags of the .segments file."""
    from pyAudioAnalysis import audioTrainTest as at
    from pyAudioAnalysis import MidTermFeatures as mtf
    from pyAudioAnalysis import audioBasicIO as io
    fs, x = io.read_audio_file(data(wav))
    x = io.stereo_to_mono(x)
    models = [at.load_model(data(os.path.join("models", n))) for n in ("svm_rbf_speaker_10", "svm_rbf_speaker_male_female")]
    mid, _, _ = mtf.mid_feature_extraction(x, fs, mid_window * fs, mid_step * fs, round(fs * 0.05), round(fs * 0.05))
    blocks = [mid]
    for clf, mean, std, names, _, _, _, _, _ in models:
        P = np.empty((len(names), mid.shape[1]))
        for i in range(mid.shape[1]):
            P[:, i] = at.classifier_wrapper(clf, "svm_rbf", (mid[:, i] - mean) / std)[1] + 1e-4
        blocks.append(P)
    s0, s1, labs = ref_seg.read_segmentation_gt(data(wav.replace(".wav", ".segments")))
    order = sorted(set(labs))                        # a stable class order (the reference's follows string hashing)
    flags, names = ref_seg.segments_to_labels(s0, s1, labs, mid_step)
    flags = np.array([order.index(names[f]) for f in flags])
    return np.vstack(blocks), flags


def sk_stages(M):
    from scipy.spatial import distance
    from sklearn.preprocessing import StandardScaler
    scaler = StandardScaler()
    Z = scaler.fit_transform(M.T)
    colsum = np.sum(distance.squareform(distance.pdist(Z.T)), axis=0)
    kept = np.nonzero(colsum < 1.1 * np.mean(colsum))[0]
    return Z, scaler, colsum, kept


def sk_silhouette(Zk, cls, k):
    from scipy.spatial import distance
    a, b = np.zeros(k), np.zeros(k)
    for c in range(k):
        share = np.nonzero(cls == c)[0].shape[0] / float(len(cls))
        if share < 0.020:
            continue
        mine = Zk[cls == c, :]
        a[c] = np.mean(distance.pdist(mine.T)) * share
        cand = []
        for c2 in range(k):
            if c2 != c:
                share2 = np.nonzero(cls == c2)[0].shape[0] / float(len(cls))
                cand.append(np.mean(distance.cdist(mine, Zk[cls == c2, :])) * (share + share2) / 2.0)
        b[c] = min(cand)
    sil = np.array([(b[c] - a[c]) / (max(b[c], a[c]) + 1e-5) for c in range(k)])
    return a, b, sil


def close(x, ref):
    return np.max(np.abs(np.asarray(x) - np.asarray(ref))) <= TIGHT * max(np.max(np.abs(ref)), 1.0)


def hmm_run(Z, labels):
    """(states, margin) or None when the model is degenerate."""
    if len(np.unique(labels)) != labels.max() + 1:
        return None
    with np.errstate(all="ignore"):
        priors, trans, means, cov = hmm_ref.train_statistics(Z.T, labels)
        if not np.all(np.isfinite(trans)) or np.any(cov <= 0):
            return None
        _, states, margins = hmm_ref.decode(priors, trans, means, cov, Z)
    return states, float(margins.min())


def run_k(Zk, Z, k, seed, need_hmm):
    """One k from one seed: None when a floor is missed or the restatement and scikit-learn disagree."""
    from sklearn.cluster import KMeans, kmeans_plusplus
    init, _ = kmeans_plusplus(Zk, k, random_state=seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = KMeans(n_clusters=k, init=init, n_init=1).fit(Zk)
    r = diar_ref.kmeans(Zk, k, init)
    if r["margin"] < DIST_FLOOR or not np.array_equal(r["labels"], km.labels_) or r["n_iter"] != km.n_iter_:
        return None
    if not close(r["centers"], km.cluster_centers_) or not close(r["inertia"], km.inertia_):
        return None
    a, b, sil = sk_silhouette(Zk, km.labels_, k)
    s = diar_ref.silhouette(Zk, r["labels"], k)
    if s["b_margin"] < DIST_FLOOR or not (close(s["a"], a) and close(s["b"], b) and close(s["sil"], sil)):
        return None
    out = {"seed": seed, "init": init, "labels": km.labels_.astype(np.int16), "centers": km.cluster_centers_, "n_iter": km.n_iter_,
           "inertia": km.inertia_, "a": a, "b": b, "sil": sil, "km_margin": r["margin"], "b_margin": s["b_margin"],
           "pair_sums": diar_ref.pair_sums(Zk, km.labels_, k)}
    if need_hmm:
        h = hmm_run(Z, km.labels_)
        if h is None or h[1] < HMM_FLOOR:
            return None
        out["hmm_states"], out["hmm_margin"] = h[0].astype(np.int16), h[1]
    return out


def make_case(name, M, flags_gt, ref_seg, first_seed, hmm_ks=(4, 9), good_k4=False):
    from scipy.signal import medfilt
    Z, scaler, colsum, kept = sk_stages(M)
    Zr, mean, var, scale = diar_ref.standardize(M)
    kept_r, colsum_r, kept_margin = diar_ref.kept_dimensions(Zr)
    assert close(Zr, Z) and np.array_equal(kept, kept_r) and close(colsum_r, colsum), name
    assert kept_margin >= DIST_FLOOR, (name, kept_margin)
    Zk = np.ascontiguousarray(Z[:, kept])
    g = {"kind": np.array("diar"), "M": M, "mean": scaler.mean_, "scale": scaler.scale_, "z_sample": Z[::7],
         "kept_dims": kept.astype(np.int32), "colsum": colsum, "kept_margin": np.array(kept_margin), "ks": np.array(KS),
         "hmm_ks": np.array(hmm_ks, dtype=np.int64)}
    if flags_gt is not None:
        g["flags_gt"] = flags_gt.astype(np.int16)
    scores = []
    for k in KS:
        need_hmm = k in hmm_ks
        for seed in range(first_seed, first_seed + 200):
            r = run_k(Zk, Z, k, seed, need_hmm)
            if r is None:
                continue
            if need_hmm:
                r["cls"] = medfilt(r["hmm_states"].astype(np.float64), 5)
                if flags_gt is not None:
                    r["purity"] = np.array(ref_seg.evaluate_speaker_diarization(r["cls"], flags_gt))
                    if good_k4 and k == 4 and r["purity"].min() < 0.9:
                        continue
            break
        else:
            raise SystemExit("%s: no usable seed for k = %d" % (name, k))
        for key, v in r.items():
            g["k%d_%s" % (k, key)] = np.asarray(v)
        scores.append(np.mean(r["sil"]))
        print("  %s k=%d seed=%d n_iter=%d margins km %.2e b %.2e%s" % (
            name, k, r["seed"], r["n_iter"], r["km_margin"], r["b_margin"],
            "  hmm %.2e purity %s" % (r["hmm_margin"], r.get("purity")) if need_hmm else ""))
    top = np.sort(scores)[-2:]
    assert top[1] - top[0] >= DIST_FLOOR, (name, "imax", top)
    g["scores"] = np.array(scores)
    g["imax"] = np.array(int(np.argmax(scores)))
    g["imax_margin"] = np.array(top[1] - top[0])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **g)
    size = os.path.getsize(path)
    assert size < 1000000, (name, size)
    print("wrote %s: D x N = %s, kept %d, imax %d, %d bytes" % (name, M.shape, len(kept), int(g["imax"]), size))


def synthetic(seed, n=700, d=40, constant_row=False):
    """Planted clusters (5 large, one of 10 windows: under the 2 % share), a block of 24 exactly repeated windows."""
    rng = np.random.default_rng(seed)
    sizes = [int(n * f) for f in (0.28, 0.24, 0.2, 0.14)]
    sizes += [n - sum(sizes) - 10, 10]
    means = rng.standard_normal((len(sizes), d)) * 3.0
    means[-1] += 12.0
    path = np.concatenate([np.full(s, i) for i, s in enumerate(sizes)])
    path = path[np.argsort(np.repeat(rng.permutation(n // 10), 10), kind="stable")]    # runs of ten windows
    X = means[path] + rng.standard_normal((n, d))
    X[n // 2 - 12:n // 2 + 12] = X[n // 2 - 12]
    M = X.T.copy()
    if constant_row:
        M[d // 2] = 3.25
    return M


def main():
    if not load_reference.reference_available():
        raise SystemExit("the reference tree is needed")
    ref_seg = load_reference.load_segmentation()
    os.makedirs(OUT, exist_ok=True)
    M, flags = reference_matrix(ref_seg, "diarizationExample.wav", 1.0, 0.1)
    make_case("diar_example", M, flags, ref_seg, 0, good_k4=True)
    M, flags = reference_matrix(ref_seg, "diarizationExample.wav", 2.0, 0.2)
    make_case("diar_example_2s", M, flags, ref_seg, 0)
    M, flags = reference_matrix(ref_seg, "diarizationExample2.wav", 1.0, 0.1)
    make_case("diar_example2", M, flags, ref_seg, 0)
    make_case("diar_synth", synthetic(5), None, ref_seg, 0, hmm_ks=(6, 9))
    make_case("diar_const", synthetic(6, n=300, d=12, constant_row=True), None, ref_seg, 0, hmm_ks=())


if __name__ == "__main__":
    main()
