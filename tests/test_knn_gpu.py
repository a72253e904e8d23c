"""GPU tests of the k-nearest-neighbour classifier (kernels_knn.hpp) and the "knn" model type of the classification
drop-ins, against the knn_* goldens (the unmodified reference, scripts/make_knn_golden.py) and the NumPy restatement with
the documented (squared distance, index) order (tests/knn_ref.py)."""
import contextlib
import ctypes as C
import io
import tempfile

import numpy as np
import pytest

import knn_ref
from conftest import golden_files, golden_id
from pyaudioanalysis_amd import MidTermFeatures, _ffi, audioSegmentation, audioTrainTest

pytestmark = pytest.mark.gpu


def _load(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def _model(g):
    return audioTrainTest.Knn(g["features"], g["labels"], int(g["neighbors"]))


def _by_case(case):
    return [f for f in golden_files("knn") if str(np.load(f, allow_pickle=False)["case"]) == case]


_ambiguous = knn_ref.ambiguous_vectors


def _neighbours_agree(nb, want, features, X, exact):
    """Equal neighbour lists; where distances are not exact, equal up to the order of neighbours whose squared distances
    agree to 1e-12 (the kernel and NumPy sum the squares in different orders)."""
    if exact:
        assert np.array_equal(nb, want)
        return
    D = knn_ref.squared_distances(features, X)
    for v in range(nb.shape[0]):
        if np.array_equal(nb[v], want[v]):
            continue
        assert sorted(nb[v].tolist()) == sorted(want[v].tolist()), v
        d = D[v, nb[v]]
        assert np.all(np.abs(d - D[v, want[v]]) <= 1e-12 * np.maximum(d, 1e-300)), v


@pytest.mark.parametrize("path", golden_files("knn"), ids=golden_id)
def test_knn_kernel_matches_reference_and_restatement(gpu_lib, path):
    g = _load(path)
    k = int(g["neighbors"])
    model = audioTrainTest.knn_model(_model(g))
    labels, P, nb = model.predict(g["mid"], g["mean"], g["std"], neighbors=True)
    X = (g["mid"].T - g["mean"]) / g["std"]
    amb = g["ref_ambiguous"]
    # the restatement's order is the kernel's: labels and P bit for bit on every vector
    assert np.array_equal(labels, g["want_labels"]) and np.array_equal(P, g["want_P"])
    _neighbours_agree(nb, g["want_nb"], g["features"], X, exact=str(g["case"]) == "ties")
    # the reference, wherever its argsort defines the vote set
    assert np.array_equal(labels[~amb], g["ref_labels"][~amb]) and np.array_equal(P[~amb], g["ref_P"][~amb])
    print("%s: %d vectors, %d ambiguous (k = %d)" % (golden_id(path), X.shape[0], int(amb.sum()), k))
    # the public one-vector forms give the same answers
    for v in range(0, X.shape[0], max(1, X.shape[0] // 9)):
        cid, p = audioTrainTest.classifier_wrapper(_model(g), "knn", X[v])
        assert cid == labels[v] and np.array_equal(p, P[v])
        cid, p = _model(g).classify(X[v])
        assert cid == labels[v] and np.array_equal(p, P[v])
    ids, P2 = audioTrainTest.knn_predict(_model(g), g["mid"], g["mean"], g["std"])
    assert np.array_equal(ids, labels) and np.array_equal(P2, P)


def _gt_file(g):
    tmp = tempfile.NamedTemporaryFile("w", suffix=".segments", delete=False)
    for (s, e), lab in zip(g["gt_segments"], g["gt_labels"]):
        tmp.write("%r\t%r\t%s\n" % (float(s), float(e), lab))
    tmp.close()
    return tmp.name


@pytest.mark.parametrize("path", _by_case("segment"), ids=golden_id)
def test_mid_term_classification_matches_reference(gpu_lib, path):
    g = _load(path)
    names = [str(c) for c in g["class_names"]]
    gt_file = _gt_file(g) if "gt_segments" in g else ""
    with contextlib.redirect_stdout(io.StringIO()) as printed:
        labels, class_names, acc, cm = audioSegmentation.mid_term_classification(
            g["signal"], g["fs"], _model(g), g["mean"], g["std"], names, float(g["mt_win"]), float(g["mid_step"]),
            float(g["st_win"]), float(g["st_step"]), False, False, gt_file, "knn")
    assert class_names == names
    assert labels.dtype == np.int64 and np.array_equal(labels, g["seg_labels"])
    assert acc == float(g["ref_accuracy"])
    if gt_file:
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
    # the model type is taken from the model when not given
    labels2, _ = audioSegmentation.mid_term_labels(audioSegmentation.audioBasicIO.stereo_to_mono(g["signal"]), g["fs"],
                                                   _model(g), g["mean"], g["std"], float(g["mt_win"]), float(g["mid_step"]),
                                                   float(g["st_win"]), float(g["st_step"]))
    assert np.array_equal(labels2, labels)


@pytest.mark.parametrize("path", _by_case("segment"), ids=golden_id)
def test_mid_term_file_classification_with_a_knn_model_file(gpu_lib, path, tmp_path):
    """The file-level entry point on the golden's model written in load_model_knn's format and its signal as a WAV file."""
    import pickle
    import scipy.io.wavfile as wavfile
    g = _load(path)
    model = str(tmp_path / "knn_model")
    with open(model, "wb") as f:
        for obj in (g["features"], g["labels"], g["mean"], g["std"], [str(c) for c in g["class_names"]], int(g["neighbors"]),
                    float(g["mt_win"]), float(g["mid_step"]), float(g["st_win"]), float(g["st_step"]), False):
            pickle.dump(obj, f)
    wav = str(tmp_path / "signal.wav")
    wavfile.write(wav, int(g["fs"]), g["signal"])
    gt_file = _gt_file(g) if "gt_segments" in g else ""
    with contextlib.redirect_stdout(io.StringIO()):
        labels, class_names, acc, cm = audioSegmentation.mid_term_file_classification(wav, model, "knn", False, gt_file)
    assert np.array_equal(labels, g["seg_labels"]) and acc == float(g["ref_accuracy"])
    assert class_names == [str(c) for c in g["class_names"]]


@pytest.mark.parametrize("path", _by_case("file"), ids=golden_id)
def test_file_classification_matches_reference(gpu_lib, path):
    g = _load(path)
    pos = 0
    args = (_model(g), g["mean"], g["std"], float(g["mt_win"]), float(g["mid_step"]), float(g["st_win"]), float(g["st_step"]),
            bool(g["compute_beat"]))
    sigs = []
    for n, cid, prob in zip(g["lengths"], g["ref_ids"], g["ref_proba"]):
        sig = g["signals"][pos:pos + int(n)]
        pos += int(n)
        sigs.append(sig)
        ours, p = audioTrainTest.file_classification_signal(sig, g["fs"], *args, "knn")
        print("file of %d samples: class %s (reference %s), P %s (reference %s)" % (n, ours, cid, p, prob))
        assert ours == cid and np.array_equal(p, prob)
    ids, proba = audioTrainTest.file_classification_signals(sigs, int(g["fs"]), *args, "knn")
    assert np.array_equal(ids, g["ref_ids"]) and np.array_equal(proba, g["ref_proba"])


def test_file_classification_batch_equals_single_calls(gpu_lib):
    g = _load(_by_case("file")[0])
    rng = np.random.default_rng(12)
    fs = int(g["fs"])
    sigs = []
    for i in range(120):
        n = int(rng.integers(int(0.3 * fs), int(6.5 * fs)))          # some shorter than the 1 s mid-term window
        t = np.arange(n) / fs
        x = 6000 * np.sin(2 * np.pi * rng.uniform(80, 2000) * t) * (1 + np.sin(2 * np.pi * rng.uniform(0.5, 4) * t))
        x += rng.normal(0, rng.uniform(50, 3000), n)
        sigs.append(np.clip(x, -32768, 32767).astype(np.int16))
    sigs[9] = np.zeros(3 * fs, dtype=np.int16)                         # a silent clip
    args = (_model(g), g["mean"], g["std"], float(g["mt_win"]), float(g["mid_step"]), float(g["st_win"]),
            float(g["st_step"]), bool(g["compute_beat"]))
    ids, proba = audioTrainTest.file_classification_signals(sigs, fs, *args, "knn")
    for i, s in enumerate(sigs):
        cid, p = audioTrainTest.file_classification_signal(s, fs, *args, "knn")
        assert cid == ids[i] and np.array_equal(p, proba[i]), i


def _check_against_restatement(F, labels, k, feats, mean, std, what, ld=None):
    X = (feats.T - mean) / std
    model = audioTrainTest.knn_model(audioTrainTest.Knn(F, labels, k))
    if ld is None:
        got, P, nb = model.predict(feats, mean, std, neighbors=True)
    else:                                                         # a matrix with ld > n_vec through the C ABI
        n_dims, n_vec = feats.shape
        M = np.zeros((n_dims, ld))
        M[:, :n_vec] = feats
        got = np.empty(n_vec, dtype=np.int32)
        P = np.empty((n_vec, model.n_classes))
        nb = np.empty((n_vec, k), dtype=np.int32)
        _ffi.check(_ffi.lib().paa_knn_predict_f64(model.handle, _ffi.as_f64p(M), n_dims, ld, n_vec, _ffi.as_f64p(mean),
                                                  _ffi.as_f64p(std), got.ctypes.data_as(_ffi.c_i32p), _ffi.as_f64p(P),
                                                  nb.ctypes.data_as(_ffi.c_i32p)))
    want, wP, wnb = knn_ref.classify(F, labels, k, X)
    amb = _ambiguous(F, labels, k, X)
    # the vectors set aside are capped: a stated share, which knn_ref alone keeps on the CPU (test_model_edges_ref_cpu.py)
    assert int(amb.sum()) <= knn_ref.AMBIGUOUS_CAP * X.shape[0], (what, int(amb.sum()), X.shape[0])
    ok = ~amb
    assert np.array_equal(got[ok], want[ok]) and np.array_equal(P[ok], wP[ok])
    _neighbours_agree(nb[ok], wnb[ok], F, X[ok], exact=False)
    print("%s: %d vectors, %d ambiguous, labels used %s" % (what, X.shape[0], int(amb.sum()), np.unique(got).tolist()))
    return got, P


@pytest.mark.parametrize("name", sorted(knn_ref.SHAPES))
def test_knn_kernel_matches_restatement_on_shipped_shapes(gpu_lib, name):
    F, labels, k, feats, mean, std = knn_ref.shape_case(name)
    _check_against_restatement(F, labels, k, feats, mean, std, name)


@pytest.mark.parametrize("name", sorted(knn_ref.EDGES))
def test_knn_kernel_edges(gpu_lib, name):
    n_train, n_dims, n_classes, k, n_vec, ld = knn_ref.EDGES[name]
    F, labels, k, feats, mean, std = knn_ref.edge_case(name)
    got, P = _check_against_restatement(F, labels, k, feats, mean, std, name, ld=ld)
    assert P.shape == (n_vec, n_classes)


def test_nan_query_returns(gpu_lib):
    """A zero std makes a query NaN: documented answer P = 0, label 0, no neighbours.  The two columns next to it are
    (2 - 1) / 0 = inf: every squared distance is inf, so the neighbours are the first k rows in index order."""
    F, labels, k = knn_ref.seeded(100, 5, 3, 4, 9)
    model = audioTrainTest.knn_model(audioTrainTest.Knn(F, labels, k))
    feats = np.ones((5, 3))
    std = np.ones(5)
    std[2] = 0.0
    feats[2, 1] = 1.0                           # (1 - 1) / 0 = NaN; the other columns (x / 0 = inf) are inf
    feats[2, [0, 2]] = 2.0
    got, P, nb = model.predict(feats, np.ones(5), std, neighbors=True)
    assert got[1] == 0 and np.all(P[1] == 0) and np.all(nb[1] == -1)
    assert got.shape == (3,) and P.shape == (3, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        X = (feats.T - np.ones(5)) / std
    want, wP, wnb = knn_ref.classify(F, labels, k, X[[0, 2]])
    assert np.array_equal(wnb, np.tile(np.arange(k), (2, 1)))
    for col, w in zip((0, 2), range(2)):
        assert got[col] == want[w] and np.array_equal(P[col], wP[w]) and np.array_equal(nb[col], wnb[w]), col


def test_one_hour_clip_through_the_device_path(gpu_lib):
    """A 1-hour clip at the shipped models' steps through mid_term_labels (the mid-term matrix goes from the plan straight
    into the kNN kernel) against the host-buffer path and, on a seeded sample, against the restatement; the model has
    knn_movie8class's shape."""
    fs = 16000
    rng = np.random.default_rng(5)
    n = 3600 * fs
    t = np.arange(n, dtype=np.float64) / fs
    x = 8000 * np.sin(2 * np.pi * 220 * t * (1 + 0.3 * np.sin(2 * np.pi * t / 97))) * (0.5 + 0.5 * np.sin(2 * np.pi * t / 13))
    x += rng.normal(0, 1500, n) * (np.sin(2 * np.pi * t / 41) > 0)
    sig = np.clip(x, -32768, 32767).astype(np.int16)
    del x, t
    mt_win, mid_step, st_win, st_step = 1.0, 1.0, 0.05, 0.05
    mid, _, _ = MidTermFeatures.mid_feature_extraction(sig, fs, mt_win * fs, mid_step * fs, round(fs * st_win),
                                                       round(fs * st_step))
    mean, std = mid.mean(axis=1), mid.std(axis=1)
    std[std == 0] = 1.0
    # training rows drawn from the clip's own standardised windows (plus noise), so that the neighbours are close
    Z = ((mid.T - mean) / std)
    pick_train = rng.choice(Z.shape[0], 3040, replace=True)
    F = Z[pick_train] + 0.3 * rng.standard_normal((3040, Z.shape[1]))
    labels = rng.integers(0, 8, 3040).astype(np.float64)
    labels[:8] = np.arange(8)
    model = audioTrainTest.Knn(F, labels, 9)
    labels_dev, pmax_dev = audioSegmentation.mid_term_labels(sig, fs, model, mean, std, mt_win, mid_step, st_win, st_step,
                                                             "knn")
    assert mid.shape[1] == labels_dev.shape[0] >= 3500
    labels_host, P_host = audioTrainTest.knn_predict(model, mid, mean, std)
    assert np.array_equal(labels_host, labels_dev) and np.array_equal(P_host.max(axis=1), pmax_dev)
    pick = np.sort(rng.choice(mid.shape[1], 64, replace=False))
    _check_against_restatement(F, labels, 9, mid[:, pick], mean, std, "1 h movie8class shape sample")
