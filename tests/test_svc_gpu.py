"""GPU tests of the multi-class probabilistic SVC (kernels_svc.hpp) and the classification drop-ins built on it, against
the svc_* goldens (scikit-learn and the unmodified reference, scripts/make_classify_golden.py) and the NumPy restatement
of libsvm (tests/svc_libsvm.py)."""
import contextlib
import io

import numpy as np
import pytest

import svc_libsvm
from conftest import golden_files, golden_id
from pyaudioanalysis_amd import MidTermFeatures, audioSegmentation, audioTrainTest

pytestmark = pytest.mark.gpu

NEAR_ZERO = 1e-9          # a window whose pairwise decision value is this close to 0 may vote either way
PROBA_TOL = 1e-9


def _load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _model(g):
    return audioTrainTest.SvcArrays(g["sv"], g["n_support"], g["dual_coef"], -g["rho"], g["prob_a"], g["prob_b"],
                                    g["gamma"], str(g["kernel"]), g["classes"])


def _labels_agree(ours, want, dec, what):
    """Equal labels except on windows with a pairwise decision value within NEAR_ZERO of 0 (counted and reported)."""
    near = np.min(np.abs(dec), axis=1) < NEAR_ZERO
    bad = (ours != want) & ~near
    print("%s: %d windows, %d with a decision value within %g of 0, %d of those differ"
          % (what, len(want), int(near.sum()), NEAR_ZERO, int(((ours != want) & near).sum())))
    assert not bad.any(), np.nonzero(bad)[0][:10]


MATRIX_GOLDENS = [f for f in golden_files("svc") if "mid" in np.load(f, allow_pickle=False).files]
SEGMENT_GOLDENS = [f for f in golden_files("svc") if str(np.load(f, allow_pickle=False)["case"]) == "segment"]
FILE_GOLDENS = [f for f in golden_files("svc") if str(np.load(f, allow_pickle=False)["case"]) == "file"]


@pytest.mark.parametrize("path", MATRIX_GOLDENS, ids=golden_id)
def test_svc_kernel_matches_sklearn(gpu_lib, path):
    g = _load(path)
    labels, proba = audioTrainTest.svm_predict(_model(g), g["mid"], g["mean"], g["std"])
    _labels_agree(labels, g["sk_labels"], g["sk_dec"], golden_id(path))
    err = float(np.max(np.abs(proba - g["sk_proba"])))
    print("%s: max |proba - sklearn| = %.3g" % (golden_id(path), err))
    assert err <= PROBA_TOL
    # one vector at a time through classifier_wrapper (the reference's per-window call) gives the same answers
    X = ((g["mid"].T - g["mean"]) / g["std"])
    for v in range(0, X.shape[0], max(1, X.shape[0] // 7)):
        cid, p = audioTrainTest.classifier_wrapper(_model(g), "svm_rbf", X[v])
        assert cid == labels[v] and np.array_equal(p, proba[v])


def test_linear_golden_has_tied_votes():
    g = _load([f for f in MATRIX_GOLDENS if "linear3" in f][0])
    assert int(g["n_tied_votes"]) >= 1 and str(g["kernel"]) == "linear"


@pytest.mark.parametrize("path", SEGMENT_GOLDENS, ids=golden_id)
def test_mid_term_classification_matches_reference(gpu_lib, path):
    g = _load(path)
    names = [str(c) for c in g["class_names"]]
    gt_file = ""
    if "gt_segments" in g:
        import tempfile
        tmp = tempfile.NamedTemporaryFile("w", suffix=".segments", delete=False)
        for (s, e), lab in zip(g["gt_segments"], g["gt_labels"]):
            tmp.write("%r\t%r\t%s\n" % (float(s), float(e), lab))
        tmp.close()
        gt_file = tmp.name
    with contextlib.redirect_stdout(io.StringIO()) as printed:
        labels, class_names, acc, cm = audioSegmentation.mid_term_classification(
            g["signal"], g["fs"], _model(g), g["mean"], g["std"], names, float(g["mt_win"]), float(g["mid_step"]),
            float(g["st_win"]), float(g["st_step"]), False, False, gt_file)
    assert class_names == names
    _labels_agree(np.asarray(labels), g["ref_labels"], g["sk_dec"], golden_id(path))
    if np.array_equal(np.asarray(labels), g["ref_labels"]):
        assert acc == float(g["ref_accuracy"])
        if gt_file:
            # the confusion matrix's rows / columns follow list(set(labels)) of the ground truth, a per-process order:
            # rebuild it with the reference's rules in the golden's order, and ours in ours
            s, e, lab = audioSegmentation.read_segmentation_gt(gt_file)
            flags, order_ours = audioSegmentation.segments_to_labels(s, e, lab, float(g["mid_step"]))
            order_ref = [str(c) for c in g["ref_class_names_gt"]]
            gt_names = [order_ours[f] for f in flags]

            def cm_in(order):
                pred = np.array([order.index(names[int(v)]) if names[int(v)] in order else -1 for v in labels])
                return audioSegmentation.calculate_confusion_matrix(pred, np.array([order.index(n) for n in gt_names]), order)
            assert np.array_equal(cm_in(order_ref), g["ref_cm"])
            assert np.array_equal(cm_in(order_ours), cm)
        else:
            assert cm.size == 0 and g["ref_cm"].size == 0
        seg_lines = [ln for ln in printed.getvalue().splitlines() if not ln.startswith("Overall")]
        ref_lines = [ln for ln in str(g["ref_printed"]).splitlines() if not ln.startswith("Overall")]
        assert seg_lines == ref_lines


@pytest.mark.parametrize("path", FILE_GOLDENS, ids=golden_id)
def test_file_classification_matches_reference(gpu_lib, path):
    g = _load(path)
    pos = 0
    for n, cid, prob in zip(g["lengths"], g["ref_ids"], g["ref_proba"]):
        sig = g["signals"][pos:pos + int(n)]
        pos += int(n)
        ours, p = audioTrainTest.file_classification_signal(sig, g["fs"], _model(g), g["mean"], g["std"], float(g["mt_win"]),
                                                            float(g["mid_step"]), float(g["st_win"]), float(g["st_step"]),
                                                            bool(g["compute_beat"]), "svm_rbf")
        err = float(np.max(np.abs(p - prob)))
        print("file of %d samples: class %s (reference %s), max |proba - reference| = %.3g" % (n, ours, cid, err))
        assert ours == cid and err <= PROBA_TOL


def test_file_classification_batch_equals_single_calls(gpu_lib):
    g = _load(FILE_GOLDENS[0])
    rng = np.random.default_rng(11)
    fs = int(g["fs"])
    sigs = []
    for i in range(200):
        n = int(rng.integers(int(0.3 * fs), int(6.5 * fs)))          # some shorter than the 1 s mid-term window
        t = np.arange(n) / fs
        x = 6000 * np.sin(2 * np.pi * rng.uniform(80, 2000) * t) * (1 + np.sin(2 * np.pi * rng.uniform(0.5, 4) * t))
        x += rng.normal(0, rng.uniform(50, 3000), n)
        sigs.append(np.clip(x, -32768, 32767).astype(np.int16))
    sigs[17] = np.zeros(3 * fs, dtype=np.int16)                        # a silent clip
    args = (_model(g), g["mean"], g["std"], float(g["mt_win"]), float(g["mid_step"]), float(g["st_win"]),
            float(g["st_step"]), bool(g["compute_beat"]))
    ids, proba = audioTrainTest.file_classification_signals(sigs, fs, *args)
    for i, s in enumerate(sigs):
        cid, p = audioTrainTest.file_classification_signal(s, fs, *args, "svm_rbf")
        assert cid == ids[i] and np.array_equal(p, proba[i]), i


def _synthetic(n_support, n_dims, seed, kernel="rbf", platt_scale=1.0):
    m = svc_libsvm.synthetic_model(n_support, n_dims, seed, kernel)
    m["prob_a"] = m["prob_a"] * platt_scale
    model = audioTrainTest.SvcArrays(m["support_vectors"], m["n_support"], m["dual_coef"], -m["rho"], m["prob_a"],
                                     m["prob_b"], m["gamma"], kernel, np.arange(len(n_support), dtype=np.float64))
    return m, model


# the two shipped models whose arrays are too large for a golden file run as seeded models of exactly their shape; the
# remaining cases reach the limits of the C ABI (16 classes, 256 dims, a class without support vectors) and the linear kernel
SYNTHETIC = {
    "speaker_10_shape": (svc_libsvm.SPEAKER_10_N_SUPPORT, 136, "rbf"),
    "movie8class_shape": (svc_libsvm.MOVIE8CLASS_N_SUPPORT, 136, "rbf"),
    "k16_d256": (tuple(range(5, 21)), 256, "rbf"),
    "k5_empty_class_linear": ((40, 0, 33, 17, 60), 71, "linear"),
    "k2_d1": ((9, 14), 1, "rbf"),
    # layouts training does not produce: classes ending exactly on the 16-vector LDS tiles, empty first and last classes,
    # fewer support vectors than one tile, Platt parameters that saturate every pair (r_ij clamped to 1e-7 / 1 - 1e-7)
    "k4_ends_on_tiles": ((16, 16, 5, 11), 9, "rbf"),
    "k13_ends_on_tiles_linear": ((16, 16, 3, 13, 16, 16, 16, 2, 14, 16, 16, 16, 16), 7, "linear"),
    "k7_empty_first_and_last": ((0, 12, 16, 4, 20, 9, 0), 255, "rbf"),
    "k3_five_vectors": ((2, 1, 2), 7, "rbf"),
    "k14_saturated": (tuple(range(3, 17)), 136, "rbf", 1e4),
    "k15_saturated_linear": (tuple(range(2, 17)), 9, "linear", 1e4),
}


@pytest.mark.parametrize("name", sorted(SYNTHETIC))
def test_svc_kernel_matches_restatement_on_model_shapes(gpu_lib, name):
    n_support, n_dims, kernel, *platt = SYNTHETIC[name]
    m, model = _synthetic(n_support, n_dims, 7, kernel, *platt)
    rng = np.random.default_rng(8)
    n_vec = 203                                           # not a multiple of the 32 windows of a workgroup
    mean, std = rng.normal(0, 2, n_dims), rng.uniform(0.5, 3.0, n_dims)
    feats = rng.standard_normal((n_dims, n_vec)) * std[:, None] + mean[:, None]
    labels, proba = audioTrainTest.svm_predict(model, feats, mean, std)
    X = ((feats.T - mean) / std)
    idx, want, dec = svc_libsvm.predict(m, X)
    _labels_agree(labels, idx.astype(np.float64), dec, name)
    err = float(np.max(np.abs(proba - want)))
    print("%s: %d classes, %d support vectors, max |proba - restatement| = %.3g"
          % (name, len(n_support), sum(n_support), err))
    assert err <= PROBA_TOL
    if platt:
        r = svc_libsvm.sigmoid_predict(dec, m["prob_a"], m["prob_b"])
        assert np.mean((r < 1e-7) | (r > 1 - 1e-7)) > 0.99


# ---- trained models at every class count the kernels are instantiated for ---------------------------------------------------
TRAINED_DIMS = (1, 7, 9, 136, 255, 256)
TRAINED_NVEC = (1, 33, 65, 3001)


def _trained_case(k, kernel):
    """A seeded scikit-learn SVC(probability=True) on k clusters, and windows near the centres, far outside every cluster
    (RBF values of exactly 0) and from clusters far apart (linear: clamped probabilities), as a [n_dims][n_vec] matrix."""
    sklearn_svm = pytest.importorskip("sklearn.svm")
    i = 2 * k + (kernel == "linear")
    n_dims, n_vec = TRAINED_DIMS[i % len(TRAINED_DIMS)], TRAINED_NVEC[(i // 2) % len(TRAINED_NVEC)]
    rng = np.random.default_rng(600 + i)
    centres = rng.standard_normal((k, n_dims)) * 2.0
    y = np.repeat(np.arange(k), 12)
    X = centres[y] + rng.standard_normal((y.shape[0], n_dims))
    clf = sklearn_svm.SVC(kernel=kernel, probability=True, gamma="scale", random_state=0).fit(X, y)
    n_near = max(1, n_vec - 2 * (n_vec // 3))
    W = np.concatenate([centres[rng.integers(0, k, n_near)] + 0.7 * rng.standard_normal((n_near, n_dims)),
                        1e3 * rng.standard_normal((n_vec // 3, n_dims)),
                        40.0 * centres[rng.integers(0, k, n_vec // 3)] + rng.standard_normal((n_vec // 3, n_dims))])[:n_vec]
    mean, std = rng.normal(0, 0.5, n_dims), rng.uniform(0.5, 2.0, n_dims)
    return clf, W.T * std[:, None] + mean[:, None], mean, std, W


@pytest.mark.parametrize("kernel", ["rbf", "linear"])
@pytest.mark.parametrize("k", list(range(2, 17)))
def test_svc_kernel_matches_sklearn_at_every_class_count(gpu_lib, k, kernel):
    """svc_proba_kernel<K> for every K = 2..16 (blocks of 64, 32 and 16 threads) against scikit-learn's own predict /
    predict_proba; n_dims 1..256 (partial groups of 8 lanes), n_vec 1..3 001 (partial blocks of both kernels)."""
    clf, feats, mean, std, W = _trained_case(k, kernel)
    labels, proba = audioTrainTest.svm_predict(clf, feats, mean, std)
    X = (feats.T - mean) / std
    want = clf.predict_proba(X)
    _, _, dec = svc_libsvm.predict(svc_libsvm.model_arrays(clf), X)
    _labels_agree(labels, clf.predict(X), dec, "K=%d %s" % (k, kernel))
    err = float(np.max(np.abs(proba - want)))
    print("SVC K=%d %s n_dims=%d n_vec=%d: max |proba - sklearn| = %.3g" % (k, kernel, X.shape[1], X.shape[0], err))
    assert err <= PROBA_TOL


def test_one_hour_movie8class_shape_against_restatement(gpu_lib):
    """A 1-hour clip at movie8class's steps (1 s / 1 s mid-term, 50 ms / 50 ms short-term) through the device-resident
    path (the mid-term matrix goes from the plan straight into the SVC) against the host-buffer path and, on a seeded
    sample of windows, against the restatement.  The model has movie8class's shape (8 classes, 2 273 support vectors)."""
    fs = 16000
    rng = np.random.default_rng(5)
    n = 3600 * fs
    t = np.arange(n, dtype=np.float64) / fs
    x = 8000 * np.sin(2 * np.pi * 220 * t * (1 + 0.3 * np.sin(2 * np.pi * t / 97))) * (0.5 + 0.5 * np.sin(2 * np.pi * t / 13))
    x += rng.normal(0, 1500, n) * (np.sin(2 * np.pi * t / 41) > 0)
    sig = np.clip(x, -32768, 32767).astype(np.int16)
    del x, t
    m, model = _synthetic(svc_libsvm.MOVIE8CLASS_N_SUPPORT, 136, 24)      # a seed whose labels spread over the classes
    mt_win, mid_step, st_win, st_step = 1.0, 1.0, 0.05, 0.05
    mid, _, _ = MidTermFeatures.mid_feature_extraction(sig, fs, mt_win * fs, mid_step * fs, round(fs * st_win),
                                                       round(fs * st_step))
    mean, std = mid.mean(axis=1), mid.std(axis=1)           # the clip's own statistics stand in for the model's MEANS file
    std[std == 0] = 1.0
    labels_dev, pmax_dev = audioSegmentation.mid_term_labels(sig, fs, model, mean, std, mt_win, mid_step, st_win, st_step)
    assert mid.shape[1] == labels_dev.shape[0] >= 3500
    labels_host, proba_host = audioTrainTest.svm_predict(model, mid, mean, std)
    assert np.array_equal(labels_host, labels_dev) and np.array_equal(proba_host.max(axis=1), pmax_dev)
    pick = np.sort(rng.choice(mid.shape[1], 48, replace=False))
    X = ((mid[:, pick].T - mean) / std)
    idx, proba, dec = svc_libsvm.predict(m, X)
    _labels_agree(labels_host[pick], idx.astype(np.float64), dec, "1 h movie8class-shape sample")
    err = float(np.max(np.abs(proba_host[pick] - proba)))
    print("1 h movie8class shape: %d windows, classes used %s, max |proba - restatement| = %.3g"
          % (mid.shape[1], np.unique(labels_host).tolist(), err))
    assert err <= PROBA_TOL
